"""GPU parity of the coalesced-batches entry point (dfmi_filter_project_batches,
include/dfmi.h): many small batches -- the reference pulls 1024-row batches
(csv_sql.rs:49, :60-62) -- in ONE launch, each batch's output exactly the
oracle's for that batch alone (one output batch per input batch, 0-row
batches included), and on an error the batches before the failing one
complete, the failing one reporting the oracle's error for it."""
import numpy as np
import pytest

from datafusion_amd._abi import DFMI_FLAG_EXT_GATHER_ALL, DFMI_FLAG_EXT_UTF8_COMPARE
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.engine import engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator, Utf8
from oracle_ffi import oracle_filter_project
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

SIZES = [1024] * 40 + [0, 1, 63, 64, 65, 1023, 1025, 4095, 4096, 4097, 20_000, 100_003, 0, 7] + [1024] * 30


def make_batches(sizes, seed=1, nullable_every=3, utf8=True):
    """Batches of a (Float64, nullable in every `nullable_every`-th batch),
    b, c (Float64) and s (Utf8)."""
    rng = np.random.default_rng(seed)
    fields = [Field("a", DataType.Float64, True), Field("b", DataType.Float64, False),
              Field("c", DataType.Float64, False)]
    if utf8:
        fields.append(Field("s", DataType.Utf8, False))
    s = Schema(fields)
    words = [b"", b"w17", b"alpha", b"\xe2\x82\xac", b"x" * 40] + [b"w%d" % i for i in range(30)]
    out = []
    for i, n in enumerate(sizes):
        valid = (rng.random(n) >= 0.2) if (nullable_every and i % nullable_every == 0) else None
        cols = [Array.from_numpy(DataType.Float64, rng.random(n), valid),
                Array.from_numpy(DataType.Float64, rng.random(n)),
                Array.from_numpy(DataType.Float64, rng.random(n))]
        if utf8:
            cols.append(Array.from_strings([words[j] for j in rng.integers(0, len(words), n)]))
        out.append(RecordBatch(s, cols))
    return s, out


def host_into(p, cp, batches, flags, pinned, shift=64):
    """dfmi_filter_project_host_batches_into over host batches, the outputs in
    a caller-owned block -- pinned (torch's pinned allocator: the kernel writes
    it in place) or pageable (staged + copied by the library) -- at a 64-byte
    (not 256-byte) aligned address; the glue builds the RecordBatches."""
    import torch
    eng = engine()
    prep = eng._host_batches_prepare(p, cp, batches, flags)
    block, outs = eng._host_batches_block(prep)
    n = block.numel()
    raw = torch.empty(n + shift + 256, dtype=torch.uint8, pin_memory=pinned)
    a = (-raw.data_ptr()) % 256 + shift
    block = raw[a:a + n]
    assert block.data_ptr() % 64 == 0
    block.fill_(0xCD)  # stale bytes must not leak into the results
    res = eng._host_batches_into_call(prep, (block, outs))
    rbs, err = eng._host_batches_into_finish(prep, res, Schema.empty(), (block, outs))
    return [rb.columns for rb in rbs], err


def check(schema, batches, pred_e, proj_e, flags=0, host=False):
    """Device batched results == the oracle batch by batch, or the first
    failing batch with the oracle's error (batches before it complete).
    host: the batches stay in host memory (dfmi_filter_project_host_batches);
    "pinned" / "pageable": ..._into with a caller-owned output block."""
    p = compile_scalar_expr(None, pred_e, schema, flags) if pred_e is not None else None
    cp = [compile_scalar_expr(None, e, schema, flags) for e in proj_e]
    if host in ("pinned", "pageable"):
        got, err = host_into(p, cp, [b.to("cpu") for b in batches], flags, host == "pinned")
    elif host:
        got, err = engine().filter_project_host_batches(p, cp, [b.to("cpu") for b in batches], flags)
    else:
        dbs = [b.to(engine().device) for b in batches]
        got, err = engine().filter_project_batches(p, cp, dbs, flags)
    for i, b in enumerate(batches):
        try:
            ref = oracle_filter_project(schema, b, pred_e, proj_e, flags)
        except ExecutionError as e:
            assert err is not None and err.failed_batch == i, (i, e, err)
            assert (err.kind, err.message) == (e.kind, e.message)
            assert len(got) == i
            return i
        assert i < len(got), (i, err)
        assert len(got[i]) == len(ref)
        for d, (name, r) in zip(got[i], ref):
            assert_same(d.cpu(), r, "batch %d %s" % (i, name))
    assert err is None, err
    return None


@pytest.mark.parametrize("host", [False, True, "pinned", "pageable"])
def test_c2_query_many_batches(host):
    s, bs = make_batches(SIZES)
    pred = BinaryExpr(BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.3))), Operator.And,
                      BinaryExpr(Column(1), Operator.Lt, Literal(Float64(0.7))))
    projs = [Column(0), Column(1), BinaryExpr(BinaryExpr(Column(0), Operator.Multiply, Column(1)), Operator.Plus,
                                              Column(2))]
    assert check(s, bs, pred, projs, host=host) is None
    # FilterRelation output (every column, Utf8 gathered)
    assert check(s, bs, pred, [], host=host) is None


@pytest.mark.parametrize("host", [False, True, "pinned", "pageable"])
def test_utf8_equality_and_gather_many_batches(host):
    s, bs = make_batches(SIZES, seed=2)
    pred = BinaryExpr(Column(3), Operator.Eq, Literal(Utf8("w17")))
    assert check(s, bs, pred, [Column(3), Column(0)], DFMI_FLAG_EXT_UTF8_COMPARE, host=host) is None
    pred = BinaryExpr(Column(0), Operator.Lt, Literal(Float64(0.5)))
    assert check(s, bs, pred, [Column(3), Column(2)], host=host) is None


@pytest.mark.parametrize("host", [False, True, "pinned", "pageable"])
def test_projection_only_many_batches(host):
    """No predicate: dense kernel per batch, null propagation, passthrough."""
    s, bs = make_batches(SIZES, seed=3)
    projs = [BinaryExpr(Column(0), Operator.Plus, Column(1)), Column(2), Column(3),
             BinaryExpr(Column(0), Operator.Lt, Column(1))]
    assert check(s, bs, None, projs, host=host) is None


@pytest.mark.parametrize("host", [False, True, "pinned", "pageable"])
def test_error_in_a_middle_batch(host):
    """DivideByZero in batch 57 only: batches 0..56 are returned, batch 57
    raises the oracle's error."""
    s, bs = make_batches([1024] * 80, seed=4, utf8=False)
    b = bs[57].columns[1].cpu()
    v = np.array(b.numpy_values())
    v[500] = 0.0
    bs[57] = RecordBatch(s, [bs[57].columns[0], Array.from_numpy(DataType.Float64, v), bs[57].columns[2]])
    pred = BinaryExpr(Column(2), Operator.GtEq, Literal(Float64(0.0)))
    projs = [BinaryExpr(Column(0), Operator.Divide, Column(1))]
    assert check(s, bs, pred, projs, host=host) == 57
    # not selected in batch 57 -> no error at all
    v2 = np.array(bs[57].columns[2].cpu().numpy_values())
    v2[500] = -1.0
    bs[57] = RecordBatch(s, [bs[57].columns[0], bs[57].columns[1], Array.from_numpy(DataType.Float64, v2)])
    assert check(s, bs, pred, projs, host=host) is None


@pytest.mark.parametrize("host", [False, True, "pinned", "pageable"])
def test_static_error_fails_batch_zero(host):
    """A plan error the reference raises on every pull ("filter not supported
    for Int64", filter.rs:106-110) fails the first batch."""
    s = Schema([Field("a", DataType.Float64, False), Field("i", DataType.Int64, False)])
    rng = np.random.default_rng(5)
    bs = [RecordBatch(s, [Array.from_numpy(DataType.Float64, rng.random(n)),
                          Array.from_numpy(DataType.Int64, rng.integers(-5, 5, n))]) for n in (0, 100, 1024)]
    pred = BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.5)))
    assert check(s, bs, pred, [], host=host) == 0
    assert check(s, bs, pred, [], DFMI_FLAG_EXT_GATHER_ALL, host=host) is None  # the extension gathers Int64


@pytest.mark.parametrize("host", [False, True, "pinned", "pageable"])
def test_boolean_outputs_fall_back_to_per_batch(host):
    s, bs = make_batches([1024] * 10 + [77, 0, 3000], seed=6)
    pred = BinaryExpr(Column(0), Operator.Lt, Literal(Float64(0.8)))
    assert check(s, bs, pred, [BinaryExpr(Column(1), Operator.Gt, Column(2)), Column(1)], host=host) is None


def test_relation_coalesces_batches():
    """ExecutionContext(coalesce=M): ProjectRelation pulls up to M batches
    from its input and runs them as one launch, still returning one output
    batch per input batch in order -- the same stream as without it."""
    s, bs = make_batches([1024] * 100 + [10, 0, 5000], seed=7)
    dbs = [b.to(engine().device) for b in bs]
    sql = "SELECT a, b, a * b + c FROM t WHERE a > 0.25 AND b < 0.75"
    streams = []
    for m in (1, 32):
        ctx = ExecutionContext(coalesce=m)
        ctx.register_datasource("t", MemoryDataSource(s, dbs))
        streams.append([[c.cpu() for c in rb.columns] for rb in ctx.sql(sql)])
    assert len(streams[0]) == len(streams[1]) == len(bs)
    for a, b in zip(*streams):
        for x, y in zip(a, b):
            assert_same(x, y)


def _oracle_stream(schema, batches, pred_e, proj_e, flags=0):
    """The reference pull loop's view, batch by batch: column lists or errors."""
    out = []
    for b in batches:
        try:
            out.append([r for _, r in oracle_filter_project(schema, b, pred_e, proj_e, flags)])
        except ExecutionError as e:
            out.append(e)
    return out


def _pull_all(rel):
    """Every next() of a relation until None, continuing after errors."""
    seen = []
    for _ in range(100_000):
        try:
            b = rel.next()
        except ExecutionError as e:
            seen.append(e)
            continue
        if b is None:
            return seen
        seen.append(b)
    raise AssertionError("relation did not end")


@pytest.mark.parametrize("m", [1, 64, 256])
def test_relation_host_batches_against_oracle(m):
    """ctx.sql over csv_sql.rs:49-style HOST batches (1024 rows, plus ragged
    and empty ones) through the relations: with read-ahead M the
    ProjectRelation runs M batches per dfmi_filter_project_host_batches call
    and still hands out the oracle's batch for every pull; a DivideByZero in
    batch 57 comes after batches 0..56 and the stream goes on after it."""
    s, bs = make_batches([1024] * 100 + [10, 0, 5000, 1024, 3] + [1024] * 60, seed=11, utf8=False)
    v = np.array(bs[57].columns[1].cpu().numpy_values())
    v[500] = 0.0
    bs[57] = RecordBatch(s, [bs[57].columns[0], Array.from_numpy(DataType.Float64, v), bs[57].columns[2]])
    c = np.array(bs[57].columns[2].cpu().numpy_values())
    c[500] = 0.5  # selected
    bs[57] = RecordBatch(s, [bs[57].columns[0], bs[57].columns[1], Array.from_numpy(DataType.Float64, c)])
    ctx = ExecutionContext(coalesce=m)
    ctx.register_datasource("t", MemoryDataSource(s, bs))
    got = _pull_all(ctx.sql("SELECT a, a / b, c FROM t WHERE c >= 0.25"))
    pred = BinaryExpr(Column(2), Operator.GtEq, Literal(Float64(0.25)))
    projs = [Column(0), BinaryExpr(Column(0), Operator.Divide, Column(1)), Column(2)]
    ref = _oracle_stream(s, bs, pred, projs)
    assert len(got) == len(ref) == len(bs)
    for i, (g, r) in enumerate(zip(got, ref)):
        if isinstance(r, ExecutionError):
            assert isinstance(g, ExecutionError) and (g.kind, g.message) == (r.kind, r.message), (i, g)
            continue
        assert not isinstance(g, ExecutionError), (i, g)
        assert g.num_rows() == r[0].length
        for d, x in zip(g.columns, r):
            assert d.values.device.type == "cpu"  # host batches in, host batches out
            assert_same(d, x, "batch %d" % i)
    assert isinstance(got[57], ExecutionError)


@pytest.mark.parametrize("m", [1, 64])
def test_filter_relation_host_batches_against_oracle(m):
    """FilterRelation alone (filter.rs:46-111: every column filtered, the
    batch's schema Schema::empty()) over host batches with read-ahead M,
    including a Utf8 column, ragged and empty batches."""
    from datafusion_amd.execution.filter import FilterRelation
    from datafusion_amd.execution.relation import DataSourceRelation
    s, bs = make_batches([1024] * 40 + [7, 0, 3000] + [1024] * 20, seed=13, utf8=True)
    pred_e = BinaryExpr(Column(0), Operator.Lt, Literal(Float64(0.4)))
    rel = FilterRelation(DataSourceRelation(MemoryDataSource(s, bs)),
                         compile_scalar_expr(None, pred_e, s, DFMI_FLAG_EXT_GATHER_ALL), s, coalesce=m)
    got = _pull_all(rel)
    ref = _oracle_stream(s, bs, pred_e, [], DFMI_FLAG_EXT_GATHER_ALL)
    assert len(got) == len(ref) == len(bs)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert not isinstance(g, ExecutionError), (i, g)
        assert g.num_rows() == r[0].length and g.num_columns() == len(r)
        for d, x in zip(g.columns, r):
            assert_same(d, x, "batch %d" % i)


def test_relation_native_csv_views_coalesced(tmp_path):
    """NativeCsvDataSource(copy=False) hands out views its next pull
    overwrites: read-ahead over it must still give the copy=True stream."""
    from datafusion_amd.execution import NativeCsvDataSource
    rng = np.random.default_rng(12)
    n = 1024 * 37 + 5
    path = tmp_path / "t.csv"
    a, b, c = rng.random(n), rng.random(n), rng.random(n)
    with open(path, "w") as f:
        f.write("a,b,c\n")
        for i in range(n):
            f.write("%r,%r,%r\n" % (float(a[i]), float(b[i]), float(c[i])))
    s = Schema([Field(x, DataType.Float64, False) for x in "abc"])
    sql = "SELECT a, b, a * b + c FROM t WHERE a > 0.25 AND b < 0.75"
    streams = []
    for m, copy in ((1, True), (4, False), (256, False)):
        ctx = ExecutionContext(coalesce=m)
        ctx.register_datasource("t", NativeCsvDataSource(s, str(path), True, 1024, copy=copy))
        streams.append([[col.cpu() for col in rb.columns] for rb in ctx.sql(sql)])
    assert len(streams[0]) == 38
    for other in streams[1:]:
        assert len(other) == len(streams[0])
        for x, y in zip(streams[0], other):
            for p, q in zip(x, y):
                assert_same(p, q)


def test_into_capacity_and_alignment_errors():
    """A block smaller than dfmi_host_batches_output_bytes is refused before
    anything runs (Capacity), as is a block that is not 64-byte aligned."""
    import ctypes as C
    import torch
    from datafusion_amd import _abi
    s, bs = make_batches([1024] * 4, seed=21, utf8=False)
    p = compile_scalar_expr(None, BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.5))), s)
    cp = [compile_scalar_expr(None, Column(1), s)]
    eng = engine()
    prep = eng._host_batches_prepare(p, cp, bs, 0)
    block, outs = eng._host_batches_block(prep)
    L = _abi.lib()
    for blk, code in ((block[:block.numel() - 256], _abi.DFMI_ERR_CAPACITY), (block[8:], _abi.DFMI_ERR_INVALID_ARGUMENT)):
        err = _abi.dfmi_error()
        failed = C.c_int32(-1)
        rc = L.dfmi_filter_project_host_batches_into(eng.ctx, prep[0], prep[1], prep[2], C.cast(prep[3], C.c_void_p),
                                                     prep[5], 0, blk.data_ptr(), blk.numel(), outs.ctypes.data,
                                                     C.byref(failed), C.byref(err))
        assert rc == code and failed.value == -1, (rc, err.message)


def test_relation_results_are_block_arrays_and_keep_inputs_alive():
    """The relations' host path: output arrays are BlockArrays over one
    caller-owned pinned block per group (views made on first read), and the
    call in flight holds its input batches itself (dropping the
    relation mid-stream must not free what the worker thread still reads)."""
    import gc
    from datafusion_amd.arrow import BlockArray
    s, bs = make_batches([1024] * 600, seed=22, utf8=False)
    ctx = ExecutionContext(coalesce=256)
    ctx.register_datasource("t", MemoryDataSource(s, bs))
    rel = ctx.sql("SELECT a, b, a * b + c FROM t WHERE a > 0.25 AND b < 0.75")
    first = rel.next()
    assert all(type(c) is BlockArray for c in first.columns)
    assert "values" not in first.columns[0].__dict__  # not viewed yet
    co = rel._co
    assert co.ahead is not None and co.ahead[0] is not None  # the next group's call is in flight
    assert co.ahead[0].prep[9] == co.ahead[1]  # ... and owns its input batches
    del rel, co, ctx
    gc.collect()
    engine().drain()
    pred = BinaryExpr(BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.25))), Operator.And,
                      BinaryExpr(Column(1), Operator.Lt, Literal(Float64(0.75))))
    projs = [Column(0), Column(1), BinaryExpr(BinaryExpr(Column(0), Operator.Multiply, Column(1)), Operator.Plus,
                                              Column(2))]
    for d, (_, r) in zip(first.columns, oracle_filter_project(s, bs[0], pred, projs)):
        assert_same(d, r)


def test_a_prepared_call_owns_its_compiled_expressions():
    """A relation dropped mid-stream was the only owner of its compiled
    expressions, and their __del__ frees the programs the worker's call still
    reads through raw handles: the prepared call holds the expressions itself
    (checked before it is started) and runs without the caller's references."""
    import gc
    import weakref
    s, bs = make_batches([1024] * 8, seed=23, utf8=False)
    pred_e = BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.25)))
    proj_e = [Column(1), BinaryExpr(Column(0), Operator.Multiply, Column(2))]
    p = compile_scalar_expr(None, pred_e, s)
    cp = [compile_scalar_expr(None, e, s) for e in proj_e]
    refs = [weakref.ref(e) for e in [p] + cp]
    out_schema = Schema([Field("b", DataType.Float64, False), Field("ac", DataType.Float64, True)])
    call = engine().filter_project_host_batches_async(p, cp, bs, 0, schema=out_schema, start=False)
    del p, cp
    gc.collect()
    assert all(r() is not None for r in refs)
    results, err = call.submit().result()
    assert err is None and len(results) == len(bs)
    for rb, b in zip(results, bs):
        for d, (_, r) in zip(rb.columns, oracle_filter_project(s, b, pred_e, proj_e)):
            assert_same(d, r)


def test_host_results_outlive_their_context():
    """A dfmi_host_result may outlive its context (the pinned pool is shared
    by a context and the results it made): a context of its own, a 2,000-row
    C2 call in four 512-row chunks (DFMI_HOST_CHUNK_ROWS=512) and a 1024-row
    one, the context destroyed, then both results read, compared with numpy
    and freed. In a child process (tests/host_result_lifetime.py says why,
    and why the chunked call comes first)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, DFMI_HOST_PROFILE="1")
    env.pop("DFMI_HOST_CHUNK_ROWS", None)
    r = subprocess.run([sys.executable, os.path.join(here, "host_result_lifetime.py")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "results outlived their context" in r.stdout
    assert "dfmi host: 4 chunks of 512 rows" in r.stderr and "dfmi host: 1 chunks of 1024 rows" in r.stderr, r.stderr
