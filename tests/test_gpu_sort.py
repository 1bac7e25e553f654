"""Sort / Limit on the device (DFMI_FLAG_EXT_SORT) against a restatement of
the contract inside this file: Python's stable `sorted` over row indices with
a functools.cmp_to_key comparator built from DESIGN.md §2's rules (false <
true, integers numerically, floats by IEEE totalOrder through an integer view
of their bits, Utf8 bytewise with a prefix first, a null greater than every
value, DESC the whole comparison reversed, ties in input order). Per output
column: length, null_count, validity, the values of valid slots bit for bit,
Utf8 bytes. The device result is never compared with itself."""
import functools

import numpy as np
import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema, np_dtype
from datafusion_amd.execution import ExecutionContext, ExecutionError, MemoryDataSource
from datafusion_amd.execution.engine import engine
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Operator
from oracle_ffi import oracle_filter_project

pytestmark = pytest.mark.gpu

SORT = _abi.DFMI_FLAG_EXT_SORT
T = DataType
INTS = [T.Int8, T.Int16, T.Int32, T.Int64, T.UInt8, T.UInt16, T.UInt32, T.UInt64]
ALL_TYPES = [T.Boolean] + INTS + [T.Float32, T.Float64, T.Utf8]
SPLIT = [1000, 37, 0, 64, 1, 255, 3, 4096]  # batch sizes, cycled: bitmap words straddle batch ends


class Col:
    """One host column: values (numpy / list of bytes) and a validity mask."""

    def __init__(self, t, vals, valid=None):
        self.t = T(t)
        self.vals = list(vals) if self.t == T.Utf8 else np.asarray(vals, dtype=bool if self.t == T.Boolean else np_dtype(self.t))
        self.n = len(self.vals)
        self.valid = np.ones(self.n, bool) if valid is None else np.asarray(valid, bool)

    def array(self, lo, hi):
        v = self.valid[lo:hi]
        if self.t == T.Utf8:
            return Array.from_strings([s if ok else None for s, ok in zip(self.vals[lo:hi], v)])
        return Array.from_numpy(self.t, self.vals[lo:hi], None if v.all() else v)

    def take(self, idx):
        vals = [self.vals[i] for i in idx] if self.t == T.Utf8 else self.vals[np.asarray(idx, dtype=np.int64)]
        return Col(self.t, vals, self.valid[np.asarray(idx, dtype=np.int64)])

    @staticmethod
    def of(a):
        a = a.cpu()
        return Col(a.data_type, a.numpy_values(), a.valid_mask())


def sizes_for(n, split):
    if not split:
        return [n]
    out, i = [], 0
    while sum(out) < n:
        out.append(min(SPLIT[i % len(SPLIT)], n - sum(out)))
        i += 1
    return out + [0]  # (and a trailing empty batch)


def batches_of(cols, sizes):
    schema = Schema([Field("c%d" % j, c.t, True) for j, c in enumerate(cols)])
    out, lo = [], 0
    for s in sizes:
        out.append(RecordBatch(schema, [c.array(lo, lo + s) for c in cols]))
        lo += s
    return out


# ---- the restatement
def total_order_key(x):
    """IEEE totalOrder as a signed integer, through the integer view of the bits."""
    bits = np.asarray(x).view(np.int32 if np.asarray(x).dtype == np.float32 else np.int64).astype(object)
    top = 1 << (31 if np.asarray(x).dtype == np.float32 else 63)
    return [int(b) if b >= 0 else -(int(b) + top) - 1 for b in bits]  # -0.0 -> -1, -NaN lowest


def comparable(col):
    """Per row None (null) or a Python value whose < is the key order."""
    if col.t == T.Utf8:
        vals = [bytes(s) for s in col.vals]
    elif col.t in (T.Float32, T.Float64):
        vals = total_order_key(col.vals)
    else:
        vals = [int(v) for v in col.vals]
    return [v if ok else None for v, ok in zip(vals, col.valid)]


def expected_order(cols, keys, limit=None):
    """Row indices in the contract's order: keys = [(column index, asc)]."""
    items = [(comparable(cols[j]), asc) for j, asc in keys]

    def cmp(i, j):
        for vals, asc in items:
            a, b = vals[i], vals[j]
            if a is None or b is None:
                c = (a is None) - (b is None)  # a null is greater than every value
            else:
                c = (a > b) - (a < b)
            if c:
                return c if asc else -c
        return 0

    order = sorted(range(cols[0].n), key=functools.cmp_to_key(cmp))  # stable: ties keep input order
    return order if limit is None else order[:limit]


def rank_np(col):
    """Per row a numpy integer whose order is the key order of the column's values: integers
    themselves, false < true as 0 < 1, floats through total_order_key's transform on the integer view of their
    bits, Utf8 the string's position among the column's distinct strings sorted as Python bytes."""
    if col.t == T.Utf8:
        vals = [bytes(s) for s in col.vals]
        pos = {s: i for i, s in enumerate(sorted(set(vals)))}
        return np.fromiter((pos[s] for s in vals), dtype=np.int64, count=col.n)
    if col.t in (T.Float32, T.Float64):
        wide = col.vals.dtype == np.float64
        bits = col.vals.view(np.int64 if wide else np.int32)
        low = (np.int64 if wide else np.int32)((1 << (63 if wide else 31)) - 1)
        return np.where(bits >= 0, bits, bits ^ low)  # b < 0: -(b + top) - 1 is b with the bits below the sign flipped
    if col.t == T.Boolean:
        return col.vals.astype(np.int8)
    return col.vals


def expected_order_np(cols, keys, limit=None):
    """expected_order for the row counts Python's `sorted` is too slow at (fixed-width keys; Utf8 keys drawn from
    a pool): per key a rank array and a null flag, ordered by one stable np.lexsort. A null ranks above every
    value (its flag is the more significant word, its rank 0); DESC reverses both words (the complement of an
    integer reverses its order without overflow). tests/test_sort_cpu.py pins it to expected_order."""
    n = cols[0].n
    lex = []  # np.lexsort: the last array is the primary key
    for j, asc in reversed(keys):
        null = ~cols[j].valid
        rank = rank_np(cols[j]).copy()
        rank[null] = 0
        lex += [rank if asc else ~rank, null if asc else ~null]
    order = np.lexsort(lex) if lex else np.arange(n)  # stable: ties keep input order
    return order if limit is None else order[:limit]


def check(out, cols, order):
    assert len(out) == len(cols)
    for a, c in zip(out, cols):
        a = a.cpu()
        e = c.take(order)
        assert a.data_type == c.t and a.length == len(order)
        assert a.null_count == int((~e.valid).sum())
        assert np.array_equal(a.valid_mask(), e.valid)
        if a.validity is not None and a.length:  # bits past length in the last word are zero
            words = a.validity.numpy()[: (a.length + 63) // 64 * 8].view(np.uint64)
            assert int(words[-1]) >> ((a.length - 1) % 64 + 1) == 0
        got = a.numpy_values()
        if c.t == T.Utf8:
            assert [g for g, ok in zip(got, e.valid) if ok] == [bytes(s) for s, ok in zip(e.vals, e.valid) if ok]
        elif c.t == T.Boolean:
            assert np.array_equal(np.asarray(got)[e.valid], e.vals[e.valid])
        else:
            u = "u%d" % np.dtype(np_dtype(c.t)).itemsize
            assert np.array_equal(np.ascontiguousarray(got).view(u)[e.valid], e.vals.view(u)[e.valid])


def run(cols, keys, limit=None, sizes=None, batches=None):
    if batches is None:
        batches = batches_of(cols, sizes or [cols[0].n])
    return engine("cuda:0").sort_batches(batches, [j for j, _ in keys], [asc for _, asc in keys], limit, SORT)


# ---- data
F64_SPECIAL = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8000000000000,
                        0xFFFFFFFFFFFFFFFF, 0xFFF0000000000123, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001,
                        0x3FF0000000000000, 0xBFF0000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF],
                       dtype=np.uint64).view(np.float64)
F32_SPECIAL = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC00000, 0xFFFFFFFF, 0xFF800123, 0x7F800000,
                        0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000,
                        0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)
STRINGS = [b"", b"a", b"a\0", b"a\0\0", b"b", b"sameprfx", b"sameprfxA", b"sameprfxB", b"sameprfx\0",
           b"sixteen-byte-pre", b"sixteen-byte-preX", b"sixteen-byte-preY", b"sixteen-byte-pr", b"\xff\xfe",
           b"\xff", b"\x00", b"\x00\x00"] + [bytes((65 + (i * 7 + k) % 26) for k in range(i)) for i in range(41)] + \
          [b"long-" + bytes((97 + k % 23) for k in range(295)), b"long-" + bytes((97 + k % 23) for k in range(294)) + b"!"]


def column(t, n, rng, nulls, distinct=None):
    """n values of type t: the type's extremes and special values, then random
    draws from a small pool (duplicates, so stability shows)."""
    t = T(t)
    if t == T.Boolean:
        pool = np.array([False, True])
    elif t in INTS:
        ii = np.iinfo(np_dtype(t))
        pool = np.array([ii.min, ii.max, ii.min + 1, ii.max - 1, 0, 1, 2, ii.max // 2, ii.max // 2 + 1], dtype=np_dtype(t))
        if ii.min < 0:
            pool = np.concatenate([pool, np.array([-1, -2, ii.min // 2], dtype=np_dtype(t))])
    elif t == T.Float64:
        pool = np.concatenate([F64_SPECIAL, rng.standard_normal(12)])
    elif t == T.Float32:
        pool = np.concatenate([F32_SPECIAL, rng.standard_normal(12).astype(np.float32)])
    else:
        pool = STRINGS
    take = (lambda p, idx: p[np.asarray(idx, dtype=np.int64)]) if isinstance(pool, np.ndarray) else \
        (lambda p, idx: [p[i] for i in idx])  # (numpy indexing keeps NaN payloads bit for bit)
    if distinct is not None:
        pool = take(pool, rng.choice(len(pool), distinct, replace=False))
    first = list(range(min(n, len(pool))))
    pick = np.concatenate([np.array(first, dtype=np.int64), rng.integers(0, len(pool), max(0, n - len(first)))])
    rng.shuffle(pick)
    vals = take(pool, pick)
    valid = rng.random(n) >= 0.2 if nulls else None
    return Col(t, vals, valid)


def entropy(t, n, rng, nulls=True):
    """n full-entropy 64-bit values (Float64, Int64 or UInt64): uniform random bit patterns, so every digit of the
    sort word varies. Float64 also gets NaNs of both signs with random payloads and F64_SPECIAL; the integers
    their extremes -- UInt64's 2^64 - 1 (twice), whose word is a null's."""
    t = T(t)
    bits = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
    if t == T.Float64:
        bits[::97] |= np.uint64(0x7FF0000000000000)  # exponent all ones, the random sign and mantissa kept: NaNs
        head = F64_SPECIAL.view(np.uint64)
    elif t == T.UInt64:
        head = np.array([2**64 - 1, 2**64 - 1, 0, 2**64 - 2, 2**63, 2**63 - 1, 1], dtype=np.uint64)
    else:
        head = np.array([2**63, 2**63 - 1, 2**64 - 1, 0, 1, 2**63 + 1], dtype=np.uint64)  # min, max, -1, 0, 1, min + 1
    bits[:min(n, len(head))] = head[:n]
    bits = rng.permutation(bits)
    return Col(t, bits.view(np_dtype(t)), rng.random(n) >= 0.2 if nulls else None)


def payloads(n, rng):
    return [column(t, n, rng, True) for t in ALL_TYPES]


@functools.lru_cache(maxsize=None)
def counts_table(n):
    """The row-count tests' table (and the default-select test's): a narrow
    nullable Int32 key with many ties, nullable payloads; the reference order
    is computed once per row count."""
    rng = np.random.default_rng(1000 + n)
    cols = [Col(T.Int32, rng.integers(-40, 40, n), rng.random(n) >= 0.1),
            Col(T.Float64, rng.standard_normal(n), rng.random(n) >= 0.3),
            Col(T.Boolean, rng.random(n) < 0.5, rng.random(n) >= 0.3),
            Col(T.Utf8, [STRINGS[i] for i in rng.integers(0, 58, n)], rng.random(n) >= 0.3),
            Col(T.Int64, np.arange(n))]
    return cols, expected_order(cols, [(0, True)])


# ---- row counts, one batch and many
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097, 100003])
def test_row_counts(n, split):
    cols, order = counts_table(n)
    check(run(cols, [(0, True)], sizes=sizes_for(n, split)), cols, order)


# ---- every key type, both directions, with and without nulls
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: t.name)
def test_key_types(t, asc, nulls):
    rng = np.random.default_rng(7 * int(t) + 2 * asc + nulls)
    n = 333
    cols = [column(t, n, rng, nulls), Col(T.Int32, np.arange(n))]
    check(run(cols, [(0, asc)], sizes=sizes_for(n, True)), cols, expected_order(cols, [(0, asc)]))


@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("t", [T.Boolean, T.Int16, T.Int64, T.Float64, T.Utf8], ids=lambda t: t.name)
def test_all_null_and_all_equal_keys(t, asc):
    rng = np.random.default_rng(5)
    n = 300
    for key in (column(t, n, rng, False).take([3] * n), Col(t, column(t, n, rng, False).vals, np.zeros(n, bool))):
        cols = [key] + payloads(n, rng)
        out = run(cols, [(0, asc)], sizes=[100, 200])
        check(out, cols, list(range(n)))  # pure stability: the input order
        check(out, cols, expected_order(cols, [(0, asc)]))


def test_sliced_input():
    rng = np.random.default_rng(11)
    n, off = 500, 13
    cols = payloads(n, rng)
    whole = batches_of(cols, [n])[0]
    cut = [(off, 200), (3, 0), (off + 200 + 5, 150), (1, 7)]  # (offset, length) slices of the same arrays
    batches = [RecordBatch(whole.schema, [a.slice(o, ln) for a in whole.columns]) for o, ln in cut]
    rows = [i for o, ln in cut for i in range(o, o + ln)]
    view = [c.take(rows) for c in cols]
    for key in (3, 10, 11, 0):  # Int32, Float64, Utf8, Boolean
        for asc in (True, False):
            out = run(view, [(key, asc)], batches=batches)
            check(out, view, expected_order(view, [(key, asc)]))


# ---- several keys
def test_three_keys_heavy_duplication():
    rng = np.random.default_rng(21)
    n = 4097
    cols = [column(T.Int64, n, rng, True, distinct=4), column(T.Utf8, n, rng, True, distinct=5),
            column(T.Float64, n, rng, True, distinct=6), Col(T.Int32, np.arange(n))]
    keys = [(0, True), (1, False), (2, True)]
    check(run(cols, keys, sizes=sizes_for(n, True)), cols, expected_order(cols, keys))


def test_eight_keys():
    rng = np.random.default_rng(22)
    n = 1500
    types = [T.Boolean, T.Int8, T.Utf8, T.Float32, T.UInt64, T.Int64, T.Float64, T.UInt16]
    cols = [column(t, n, rng, i % 2 == 0, distinct=2 if t != T.Boolean else None) for i, t in enumerate(types)]
    cols.append(Col(T.Int32, np.arange(n)))
    keys = [(i, i % 3 != 1) for i in range(8)]
    check(run(cols, keys, sizes=sizes_for(n, True)), cols, expected_order(cols, keys))


def test_payload_columns_of_every_type():
    rng = np.random.default_rng(23)
    n = 777
    cols = payloads(n, rng) + [column(t, n, rng, False) for t in (T.Boolean, T.Utf8, T.Int16)]
    cols.append(column(T.Float64, n, rng, True, distinct=9))
    keys = [(len(cols) - 1, False)]
    check(run(cols, keys, sizes=sizes_for(n, True)), cols, expected_order(cols, keys))


def test_no_keys_is_the_input_order():
    rng = np.random.default_rng(24)
    cols = payloads(200, rng)
    check(run(cols, [], sizes=[64, 0, 136]), cols, list(range(200)))
    check(run(cols, [], limit=70, sizes=[64, 0, 136]), cols, list(range(70)))


# ---- LIMIT, with the top-k prefilter forced off and on
def limit_tables():
    rng = np.random.default_rng(31)
    n = 1000
    idx = Col(T.Int32, np.arange(n))
    return {
        "f64_nulls": ([column(T.Float64, n, rng, True), idx] + payloads(n, rng)[:3], [(0, True)]),
        "f64_desc": ([column(T.Float64, n, rng, True), idx], [(0, False)]),
        "ties_past_limit": ([column(T.Int64, n, rng, False, distinct=3), idx], [(0, True)]),  # tie groups of ~333 rows
        "all_words_equal": ([Col(T.Int64, np.full(n, 42)), column(T.Int16, n, rng, True), idx], [(0, True), (1, False)]),
        "i8_nulls_desc": ([column(T.Int8, n, rng, True), column(T.Utf8, n, rng, True), idx], [(0, False), (1, True)]),
        "utf8_lead": ([column(T.Utf8, n, rng, True), idx], [(0, True)]),
        "utf8_lead_desc": ([column(T.Utf8, n, rng, True), idx], [(0, False)]),
        "bool_nulls": ([column(T.Boolean, n, rng, True), idx], [(0, True)]),
    }


LIMIT_TABLES = limit_tables()


@pytest.mark.parametrize("name", sorted(LIMIT_TABLES))
def test_limit_with_and_without_select(name, monkeypatch):
    cols, keys = LIMIT_TABLES[name]
    n = cols[0].n
    full = expected_order(cols, keys)
    monkeypatch.setenv("DFMI_DIAG", "1")
    for limit in (0, 1, 7, n - 1, n, n + 5):
        outs = []
        for select in ("0", "1"):
            monkeypatch.setenv("DFMI_SORT_SELECT", select)
            out = run(cols, keys, limit=limit, sizes=sizes_for(n, True))
            check(out, cols, full[:limit])
            outs.append(out)
        for a, b in zip(*outs):  # and the two paths agree with each other
            assert a.length == b.length and a.null_count == b.null_count


def test_default_select_at_the_largest_shape():
    cols, order = counts_table(100003)
    for limit in (100, 12000):  # below / above the default switch point's ratio
        check(run(cols, [(0, True)], limit=limit, sizes=sizes_for(100003, True)), cols, order[:limit])


# ---- through SQL
def sql_table(n=2101, zero_b=False):
    rng = np.random.default_rng(41)
    a = Col(T.Int64, rng.integers(-50, 50, n))
    b = Col(T.Int64, rng.integers(0 if zero_b else 1, 9, n))
    s = Col(T.Utf8, [STRINGS[i] for i in rng.integers(17, 40, n)])
    cols = [a, b, s]
    schema = Schema([Field("a", T.Int64, False), Field("b", T.Int64, False), Field("s", T.Utf8, False)])
    sizes = sizes_for(n, True)
    batches, lo = [], 0
    for sz in sizes:
        batches.append(RecordBatch(schema, [c.array(lo, lo + sz) for c in cols]))
        lo += sz
    return schema, cols, batches


def sql_context(schema, batches, device=True):
    ctx = ExecutionContext(flags=SORT | _abi.DFMI_FLAG_EXT_GATHER_ALL)
    ctx.register_datasource("t", MemoryDataSource(schema, [b.to("cuda:0") if device else b for b in batches]))
    return ctx


def pull_all(rel):
    out = []
    while True:
        b = rel.next()
        if b is None:
            return out
        out.append(b)


def concat(batches, ncols):
    parts = [[Col.of(b.column(j)) for b in batches] for j in range(ncols)]
    return [Col(p[0].t, [v for c in p for v in c.vals], np.concatenate([c.valid for c in p])) for p in parts]


def test_sql_where_order_by_limit():
    schema, cols, batches = sql_table()
    whole = RecordBatch(schema, [c.array(0, c.n) for c in cols])
    pred = BinaryExpr(Column(0), Operator.Gt, _lit(0))
    ref = [Col.of(a) for _, a in oracle_filter_project(schema, whole, pred, [Column(0), Column(2)],
                                                        _abi.DFMI_FLAG_EXT_GATHER_ALL)]
    rel = sql_context(schema, batches).sql("SELECT a, s FROM t WHERE a > 0 ORDER BY s DESC, a LIMIT 10")
    got = pull_all(rel)
    assert len(got) == 1 and got[0].num_rows() == 10
    check(got[0].columns, ref, expected_order(ref, [(1, False), (0, True)], 10))
    assert rel.next() is None


def _lit(v):
    from datafusion_amd.logicalplan import Int64, Literal
    return Literal(Int64(v))


def test_sql_expression_key():
    schema, cols, batches = sql_table()
    whole = RecordBatch(schema, [c.array(0, c.n) for c in cols])
    key = Col.of(oracle_filter_project(schema, whole, None, [BinaryExpr(Column(0), Operator.Plus, Column(1))])[0][1])
    for device in (True, False):
        rel = sql_context(schema, batches, device).sql("SELECT a, b FROM t ORDER BY a + b")
        got = pull_all(rel)
        assert len(got) == 1 and got[0].num_columns() == 2  # the helper column is dropped
        order = expected_order([cols[0], cols[1], key], [(2, True)])
        check(got[0].columns, cols[:2], order)


def test_sql_plain_limit_across_batches():
    schema, cols, batches = sql_table()
    for limit in (0, 1, 1000, 1050, 2101, 5000):
        got = pull_all(sql_context(schema, batches).sql("SELECT s, a FROM t LIMIT %d" % limit))
        k = min(limit, cols[0].n)
        assert sum(b.num_rows() for b in got) == k
        if k:
            check([Array_of(c) for c in concat(got, 2)], [cols[2], cols[0]], list(range(k)))
        else:
            assert got == []


def Array_of(col):
    return col.array(0, col.n)


def test_sql_key_division_by_zero_is_the_projections_error():
    schema, cols, batches = sql_table(zero_b=True)
    with pytest.raises(ExecutionError) as alone:
        pull_all(sql_context(schema, batches).sql("SELECT a / b FROM t"))
    with pytest.raises(ExecutionError) as sorted_:
        pull_all(sql_context(schema, batches).sql("SELECT a, b FROM t ORDER BY a / b LIMIT 5"))
    assert (sorted_.value.kind, sorted_.value.message) == (alone.value.kind, alone.value.message)
    assert "DivideByZero" in alone.value.kind


def test_sort_over_an_aggregate_relation():
    """Any Relation may be the input: a hand-built Sort over a GROUP BY."""
    from datafusion_amd.execution.context import Aggregate, Sort, TableScan
    from datafusion_amd.logicalplan import AggregateFunction, SortExpr
    schema, cols, batches = sql_table()
    ctx = ExecutionContext(flags=SORT | _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_GATHER_ALL)
    ctx.register_datasource("t", MemoryDataSource(schema, [b.to("cuda:0") for b in batches]))
    agg = Aggregate(TableScan("t", schema), [Column(1)], [AggregateFunction("sum", (Column(0),), T.Int64)])
    got = pull_all(ctx.execute(Sort([SortExpr(Column(1), False), SortExpr(Column(0), True)], agg)))
    assert len(got) == 1
    sums = {}
    for a, b in zip(cols[0].vals, cols[1].vals):
        sums[int(b)] = sums.get(int(b), 0) + int(a)
    groups = sorted(sums)
    ref = [Col(T.Int64, groups), Col(T.Int64, [sums[g] for g in groups])]
    check(got[0].columns, ref, expected_order(ref, [(1, False), (0, True)]))


# ---- argument errors
def test_argument_errors():
    rng = np.random.default_rng(51)
    cols = payloads(10, rng)
    eng = engine("cuda:0")
    b = batches_of(cols, [10])
    with pytest.raises(ExecutionError) as e:
        eng.sort_batches(b, [0], [True], None, 0)  # no flag
    assert e.value.kind == "InvalidArgument"
    with pytest.raises(ExecutionError) as e:
        eng.sort_batches(b, [len(cols)], [True], None, SORT)
    assert e.value.kind == "InvalidArgument"
    with pytest.raises(ExecutionError) as e:
        eng.sort_batches(b, [0] * 9, [True] * 9, None, SORT)
    assert e.value.kind == "NotImplemented" and e.value.message.startswith("device program limit: ")
