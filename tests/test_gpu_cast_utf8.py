"""GPU tests of CAST to Utf8 (DFMI_FLAG_EXT_CAST_UTF8): offsets, bytes, validity,
length and null count compared exactly.

The oracle executes no such cast, so the expected text comes from Python --
str() of an integer, `disp` of a float (tests/test_cast_utf8_cpu.py, pinned
there on round trips and on numpy's unique positional form) -- and never from
the device; what surrounds the cast (the child expression, the Selection)
comes from the oracle."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest
import torch

from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema, np_dtype, unpack_bits
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.engine import column_struct, engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.execution.projection import ProjectRelation
from datafusion_amd.logicalplan import BinaryExpr, Cast, Column, DataType, Float64, Literal, Operator
from datafusion_amd.sqlplanner import SqlToRel
from oracle_ffi import oracle_filter_project
from test_cast_utf8_cpu import disp
from test_gpu_sort import pull_all

pytestmark = pytest.mark.gpu

CAST, ANY, TO_UTF8 = _abi.DFMI_FLAG_EXT_CAST, _abi.DFMI_FLAG_EXT_CAST_ANY, getattr(_abi, "DFMI_FLAG_EXT_CAST_UTF8", 0x1000)
ON = CAST | TO_UTF8
FL = ON | _abi.DFMI_FLAG_EXT_GATHER_ALL
BOOL, I32, I64, F32, F64, U8 = (DataType.Boolean, DataType.Int32, DataType.Int64, DataType.Float32, DataType.Float64,
                                DataType.Utf8)
INTS = [DataType.Int8, DataType.Int16, DataType.Int32, DataType.Int64, DataType.UInt8, DataType.UInt16,
        DataType.UInt32, DataType.UInt64]
TYPES = [BOOL] + INTS + [F32, F64]
T = 256  # the write kernel's tile rows (csrc/format.h kTileRows)
WORST = {"Boolean": 5, "Int8": 4, "Int16": 6, "Int32": 11, "Int64": 20, "UInt8": 3, "UInt16": 5, "UInt32": 10,
         "UInt64": 20, "Float32": 48, "Float64": 327}


def text(t, v) -> bytes:
    if t == BOOL:
        return b"true" if v else b"false"
    if t == F64:
        return disp(float(v)).encode()
    if t == F32:
        return disp(np.float32(v)).encode()
    return str(int(v)).encode()


def values(t, n, seed):
    """n values of type t in which every string length of the type occurs, extremes included."""
    r = np.random.default_rng(seed)
    if t == BOOL:
        return r.integers(0, 2, n).astype(bool)
    if t in (F32, F64):
        w = 32 if t == F32 else 64
        bits = r.integers(0, 1 << w, n, dtype=np.uint64)
        return (bits.astype(np.uint32).view(np.float32) if t == F32 else bits.view(np.float64)).copy()
    dt = np_dtype(t)
    info = np.iinfo(dt)
    edge = [info.min, info.max, 0, 1]
    k = 1
    while k <= info.max:
        edge += [k, k - 1]
        if info.min < 0 and -k >= info.min:
            edge += [-k, -(k - 1)]
        k *= 10
    out = r.integers(0, 1 << 64, n, dtype=np.uint64).astype(dt)  # (wraps into the type)
    even = np.arange(0, n, 2)
    if len(even):
        out[even] = np.array([edge[(i // 2) % len(edge)] for i in even], dtype=dt)
    return out


def expected_strings(t, vals, valid):
    return [text(t, v) if ok else b"" for v, ok in zip(vals, valid)]


def check(got: Array, t, vals, valid, what=""):
    """got (a device Utf8 Array) is exactly the formatted column."""
    n = len(vals)
    want = expected_strings(t, vals, valid)
    g = got.cpu()
    assert g.data_type == U8 and g.length == n and g.offset == 0, what
    offs = g.offsets.numpy()[: n + 1]
    want_offs = np.zeros(n + 1, np.int64)
    want_offs[1:] = np.cumsum([len(s) for s in want])
    assert np.array_equal(offs, want_offs), (what, t)
    data = bytes(g.values.numpy().view(np.uint8)[: int(want_offs[-1])])
    flat = b"".join(want)
    if data != flat:
        i = next(i for i in range(n) if data[want_offs[i]:want_offs[i + 1]] != want[i])
        raise AssertionError("%s %s row %d: got %r want %r (value %r)" % (what, t, i, data[want_offs[i]:want_offs[i + 1]],
                                                                        want[i], vals[i]))
    nulls = int(n - np.sum(valid))
    assert g.null_count == nulls, (what, t)
    if nulls:
        words = g.validity.numpy().view(np.uint8)[: (n + 63) // 64 * 8]
        bits = unpack_bits(words, len(words) * 8)
        assert np.array_equal(bits[:n], np.asarray(valid, bool)) and not bits[n:].any(), (what, t)
    else:
        assert g.validity is None


def dev_array(t, vals, valid=None, offset=0):
    """A device Array of vals (with `offset` leading rows of other values: a sliced array)."""
    vals = np.asarray(vals, dtype=bool if t == BOOL else np_dtype(t))
    valid = np.ones(len(vals), bool) if valid is None else np.asarray(valid, bool)
    if offset:
        pad_v = values(t, offset, 99)
        full = Array.from_numpy(t, np.concatenate([pad_v, vals]), np.concatenate([np.arange(offset) % 2 == 0, valid]))
        a = full.slice(offset, len(vals))
    else:
        a = Array.from_numpy(t, vals, None if valid.all() else valid)
    return a.to(engine().device)


def fmt(arrays, flags=ON):
    return engine().format_utf8(arrays, flags)


def some_nulls(n, seed, p=0.3):
    return np.random.default_rng(seed).random(n) >= p


# ------------------------------------------------- 1. the entry point: row counts
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("t", TYPES, ids=[t.name for t in TYPES])
def test_every_type_and_row_count(t):
    cols = [(values(t, n, 7 + n), some_nulls(n, n) if n % 2 else np.ones(n, bool)) for n in SIZES]
    got = fmt([dev_array(t, v, ok) for v, ok in cols])
    for (v, ok), g, n in zip(cols, got, SIZES):
        check(g, t, v, ok, "n=%d" % n)


@pytest.mark.parametrize("t", [I64, F64, DataType.UInt8], ids=lambda t: t.name)
def test_past_one_scan_block_and_past_one_grid(t, monkeypatch):
    n = 40 * T + 5  # many blocks of the scan; with the grid capped at 3 workgroups every kernel loops
    v, ok = values(t, n, 11), some_nulls(n, 12)
    check(fmt([dev_array(t, v, ok)])[0], t, v, ok, "one grid")
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_FORMAT_GRID", "3")
    got = fmt([dev_array(t, v, ok), dev_array(t, v[:700])])  # two columns under the looping grid
    check(got[0], t, v, ok, "grid of 3")
    check(got[1], t, v[:700], np.ones(700, bool), "grid of 3, second column")


# ------------------------------------------------- 2. values and layout
@pytest.mark.parametrize("t", TYPES, ids=[t.name for t in TYPES])
def test_nulls_slices_and_no_validity(t):
    n = 2 * T + 41
    v = values(t, n, 21)
    lens = {len(text(t, x)) for x in v}
    if t in INTS or t == BOOL:  # every length of the type occurs
        lo = 4 if t == BOOL else 1
        assert lens == set(range(lo, WORST[t.name] + 1)), (t, lens)
    part = some_nulls(n, 22)
    none = np.zeros(n, bool)
    got = fmt([dev_array(t, v, part), dev_array(t, v, none), dev_array(t, v), dev_array(t, v, part, offset=37),
               dev_array(t, v[:100], None, offset=3)])
    check(got[0], t, v, part, "30% nulls")
    check(got[1], t, v, none, "all null")
    check(got[2], t, v, np.ones(n, bool), "no validity")
    check(got[3], t, v, part, "sliced at 37")
    check(got[4], t, v[:100], np.ones(100, bool), "sliced at 3")


def test_columns_of_different_types_and_lengths_in_one_call():
    spec = [(I64, 300), (BOOL, 70), (F64, 0), (DataType.UInt8, 1000), (F32, 257), (DataType.Int16, 1), (F64, 513)]
    cols = [(t, values(t, n, 30 + i), some_nulls(n, 40 + i) if i % 2 else np.ones(n, bool))
            for i, (t, n) in enumerate(spec)]
    got = fmt([dev_array(t, v, ok) for t, v, ok in cols])
    for (t, v, ok), g in zip(cols, got):
        check(g, t, v, ok, "mixed call")


# ------------------------------------------------- 3. floats
HAND = [1.0, 0.1, 1e21, 1e22, 1e23, 5e-324, -5e-324, 2.0 ** 53, 2.0 ** 53 - 1, 2.0 ** 53 + 2, -0.0, 0.0, 0.3, 2.5,
        123456.789, 1e-7, 0.30000000000000004, 1.7976931348623157e308, 2.2250738585072014e-308, 4194303.75, 8388607.5,
        float("inf"), float("-inf")]


def nan_bits(w):
    if w == 64:
        b = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000123,
                      0x7fffffffffffffff], np.uint64)
        return b.view(np.float64)
    b = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800123, 0x7fffffff], np.uint32)
    return b.view(np.float32)


@pytest.mark.parametrize("t", [F32, F64], ids=lambda t: t.name)
def test_float_corpus(t):
    dt = np_dtype(t)
    bound = 2.0 ** (24 if t == F32 else 53)
    around = np.concatenate([bound - 300 + np.arange(300), bound + 2 * np.arange(300), -(bound - 5 + np.arange(5))])
    prices = np.random.default_rng(5).integers(0, 10 ** 7, 3000) / 100.0
    with np.errstate(over="ignore"):
        v = np.concatenate([np.array(HAND).astype(dt), nan_bits(32 if t == F32 else 64), around.astype(dt),
                            prices.astype(dt), values(t, 6000, 51)])
    check(fmt([dev_array(t, v)])[0], t, v, np.ones(len(v), bool), "float corpus")


@pytest.mark.parametrize("t", [F32, F64], ids=lambda t: t.name)
def test_a_slice_of_subnormals_overflows_the_stage_next_to_slices_that_do_not(t):
    # rows [64, 128) and [300, 340): near-maximal strings (a 64-row slice of them is ~20 KB / ~3 KB, past the
    # 2 KB LDS image: the per-lane stores), between slices of short strings (the staged words)
    n = 3 * T
    v = (np.arange(n) % 1000 / 8.0).astype(np_dtype(t))
    tiny = np.arange(1, n + 1).astype(np.uint64 if t == F64 else np.uint32).view(np_dtype(t))  # subnormals
    for lo, hi in ((64, 128), (300, 340)):
        v[lo:hi] = tiny[lo:hi]
    v[70] = -v[70]
    ok = np.ones(n, bool)
    ok[[65, 127, 301]] = False
    check(fmt([dev_array(t, v, ok)])[0], t, v, ok, "subnormal slab")
    assert max(len(text(t, x)) for x in v) >= (320 if t == F64 else 44)


# ------------------------------------------------- 4. measure mode, capacity
def raw_call(arrays, caps, flags=ON, fill=0xAB):
    """dfmi_format_utf8_batches with data buffers of caps[i] bytes (None: measure mode), pre-filled."""
    eng = engine()
    L = _abi.lib()
    n = len(arrays)
    carr = (_abi.dfmi_column * n)(*[column_struct(a) for a in arrays])
    rows = (C.c_int64 * n)(*[a.length for a in arrays])
    outs = (_abi.dfmi_out_column * n)()
    keep = []
    for i, a in enumerate(arrays):
        offs = torch.full((a.length + 1,), -7, dtype=torch.int32, device=eng.device)
        valid = torch.zeros((a.length + 63) // 64 * 8 + 8, dtype=torch.uint8, device=eng.device)
        data = None if caps[i] is None else torch.full((caps[i] + 16,), fill, dtype=torch.uint8, device=eng.device)
        outs[i].offsets, outs[i].validity = offs.data_ptr(), valid.data_ptr()
        if data is not None:
            outs[i].data, outs[i].data_capacity = data.data_ptr(), caps[i]
        keep.append((offs, valid, data))
    lens = (C.c_int64 * n)(*([-1] * n))
    err = _abi.dfmi_error()
    L.dfmi_context_set_stream(eng.ctx, C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    rc = L.dfmi_format_utf8_batches(eng.ctx, carr, rows, n, outs, lens, flags, C.byref(err))
    torch.cuda.synchronize()
    return rc, err.message.decode(), outs, list(lens), keep


def test_measure_then_exact_write_and_one_byte_short():
    specs = [(F64, values(F64, 700, 61)), (I64, values(I64, 300, 62)), (F32, values(F32, 129, 63))]
    ok = [some_nulls(len(v), 64 + i) for i, (_, v) in enumerate(specs)]
    arrays = [dev_array(t, v, o) for (t, v), o in zip(specs, ok)]
    need = [sum(len(s) for s in expected_strings(t, v, o)) for (t, v), o in zip(specs, ok)]
    rc, msg, outs, lens, keep = raw_call(arrays, [None] * 3)
    assert rc == _abi.DFMI_OK and lens == need
    for i, ((t, v), o) in enumerate(zip(specs, ok)):  # measure mode wrote the offsets
        want = np.concatenate([[0], np.cumsum([len(s) for s in expected_strings(t, v, o)])])
        assert np.array_equal(keep[i][0].cpu().numpy(), want)
        assert (outs[i].length, outs[i].null_count, outs[i].data_length) == (len(v), int((~o).sum()), need[i])
    rc, msg, outs, lens, keep = raw_call(arrays, need)
    assert rc == _abi.DFMI_OK and lens == need
    for i, ((t, v), o) in enumerate(zip(specs, ok)):
        data = keep[i][2].cpu().numpy()
        assert bytes(data[:need[i]]) == b"".join(expected_strings(t, v, o))
        assert (data[need[i]:] == 0xAB).all()  # nothing past the exact size
    short = [need[0], need[1] - 1, need[2]]
    rc, msg, outs, lens, keep = raw_call(arrays, short)
    assert rc == _abi.DFMI_ERR_CAPACITY and lens == need
    for i in range(3):
        assert (keep[i][2].cpu().numpy() == 0xAB).all()  # no byte of any column written


def test_argument_errors():
    a = dev_array(I64, values(I64, 10, 1))
    rc, msg, _, _, _ = raw_call([a], [200], flags=CAST | ANY)
    assert rc == _abi.DFMI_ERR_NOT_IMPLEMENTED
    rc, msg, _, _, _ = raw_call([a], [200], flags=TO_UTF8)
    assert rc == _abi.DFMI_ERR_NOT_IMPLEMENTED
    s = Array.from_strings([b"a", b"bc"]).to(engine().device)
    rc, msg, _, _, _ = raw_call([s], [16])
    assert rc == _abi.DFMI_ERR_INVALID_ARGUMENT


# ------------------------------------------------- 5. round trip through the device parser
@pytest.mark.parametrize("t", [F64, F32, I64], ids=lambda t: t.name)
def test_round_trip_through_the_device_parser(t):
    if t == I64:
        v = values(I64, 3000, 71)
    else:
        w = 32 if t == F32 else 64
        with np.errstate(over="ignore"):
            v = np.concatenate([values(t, 3000, 72), np.array(HAND).astype(np_dtype(t)), nan_bits(w)])
    (s,) = fmt([dev_array(t, v)])
    schema = Schema([Field("s", U8, True)])
    flags = CAST | ANY | _abi.DFMI_FLAG_EXT_GATHER_ALL
    prog = compile_scalar_expr(None, Cast(Column(0), t), schema, flags)
    (back,) = engine().filter_project(None, [prog], RecordBatch(schema, [s]), flags)  # (a 19-digit limit row would raise)
    back = back.cpu()
    assert back.null_count == 0 and back.length == len(v)
    u = "u%d" % np.dtype(np_dtype(t)).itemsize
    got, want = np.array(back.numpy_values()).view(u), v.view(u).copy()
    if t != I64:
        want[np.isnan(v)] = 0x7ff8000000000000 if t == F64 else 0x7fc00000  # the parser's positive quiet NaN
    assert np.array_equal(got, want)


# ------------------------------------------------- 6. through the engine
def table(n, seed, null_k=True):
    r = np.random.default_rng(seed)
    k = r.integers(-10 ** 6, 10 ** 6, n)
    a, b = r.random(n), np.round(r.random(n) * 1000, 2)
    s = [b"s%d" % (i % 97) for i in range(n)]
    kv = r.random(n) > 0.2 if null_k else np.ones(n, bool)
    schema = Schema([Field("k", I64, True), Field("a", F64, True), Field("b", F64, True), Field("s", U8, True)])
    cols = [Array.from_numpy(I64, k, kv), Array.from_numpy(F64, a), Array.from_numpy(F64, b), Array.from_strings(s)]
    return schema, RecordBatch(schema, cols)


SQL = "SELECT CAST(k AS VARCHAR), CAST(a * b AS VARCHAR), s FROM t WHERE a < 0.5"
CHILDREN = [Column(0), BinaryExpr(Column(1), Operator.Multiply, Column(2)), Column(3)]
PRED = BinaryExpr(Column(1), Operator.Lt, Literal(Float64(0.5)))


def check_against_oracle(schema, batch, pred, got_cols, what):
    """got_cols: the outputs of [CAST(k), CAST(a * b), s]; the oracle runs the children and the Selection."""
    ref = [a for _, a in oracle_filter_project(schema, batch, pred, CHILDREN, FL & ~TO_UTF8)]
    for j, t in ((0, I64), (1, F64)):
        check(got_cols[j], t, ref[j].numpy_values(), ref[j].valid_mask(), what)
    g = got_cols[2].cpu()
    assert g.numpy_values() == ref[2].numpy_values() and g.length == ref[2].length, what


def slice_batch(schema, batch, lo, hi):
    cols = []
    for c in batch.columns:
        if c.data_type == U8:
            cols.append(Array.from_strings(c.numpy_values()[lo:hi]))
        else:
            cols.append(Array.from_numpy(c.data_type, c.numpy_values()[lo:hi], c.valid_mask()[lo:hi]))
    return RecordBatch(schema, cols)


def test_ctx_sql_and_without_the_flag():
    schema, batch = table(5000, 81)
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(schema, [batch.to(engine().device)]))
    (rb,) = pull_all(ctx.sql(SQL))
    assert [f.name for f in rb.schema.fields][:2] == ["CAST(#0 AS Utf8)", "CAST(#1 Multiply #2 AS Utf8)"]
    assert [f.data_type for f in rb.schema.fields] == [U8, U8, U8]
    check_against_oracle(schema, batch, PRED, rb.columns, "ctx.sql")
    ctx0 = ExecutionContext(flags=FL & ~TO_UTF8)
    ctx0.register_datasource("t", MemoryDataSource(schema, [batch.to(engine().device)]))
    with pytest.raises(ExecutionError) as e:
        pull_all(ctx0.sql(SQL))
    assert (e.value.kind, e.value.message) == ("NotImplemented", "CAST from Int64 to Utf8")


@pytest.mark.parametrize("filtered", [False, True], ids=["project", "filter+project"])
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_project_relation_coalesced_over_1024_row_batches(filtered, host):
    schema, batch = table(4 * 1024 + 333, 82)
    cuts = [0, 1024, 2048, 3072, 4096, 4096 + 333]  # a ragged last batch
    parts = [slice_batch(schema, batch, lo, hi) for lo, hi in zip(cuts, cuts[1:])]
    src = parts if host else [p.to(engine().device) for p in parts]
    ctx = ExecutionContext(flags=FL, coalesce=256)
    ctx.register_datasource("t", MemoryDataSource(schema, src))
    rel = ctx.sql(SQL if filtered else SQL.split(" WHERE")[0])
    assert isinstance(rel, ProjectRelation) and rel._format
    out = pull_all(rel)
    assert len(out) == len(parts)
    for rb, p in zip(out, parts):
        assert all(c.values.is_cuda for c in rb.columns)  # (a host batch: uploaded, device results)
        check_against_oracle(schema, p, PRED if filtered else None, rb.columns, "coalesced")
    # one pull per batch gives the same
    ctx1 = ExecutionContext(flags=FL, coalesce=1)
    ctx1.register_datasource("t", MemoryDataSource(schema, src))
    for rb, p in zip(pull_all(ctx1.sql(SQL)), parts):
        check_against_oracle(schema, p, PRED, rb.columns, "one by one")


def test_a_fused_pass_error_keeps_kind_text_and_batch():
    n = 3000
    schema = Schema([Field("k", I64, True), Field("z", I64, True)])
    k, z = np.arange(n) - 1500, np.ones(n, np.int64)
    z[2100] = 0  # batch 2, its row 52
    cuts = [0, 1024, 2048, 3000]
    parts = [RecordBatch(schema, [Array.from_numpy(I64, k[lo:hi]), Array.from_numpy(I64, z[lo:hi])]).to(engine().device)
             for lo, hi in zip(cuts, cuts[1:])]
    e = Cast(BinaryExpr(Column(0), Operator.Divide, Column(1)), U8)
    prog = compile_scalar_expr(None, e, schema, FL)
    results, err = engine().filter_project_batches(None, [prog], parts, FL)
    assert err is not None and (err.kind, err.message) == ("ArrowError(DivideByZero)", "DivideByZero")
    assert err.failed_batch == 2 and len(results) == 2 and hasattr(err, "order_key")
    for res, (lo, hi) in zip(results, zip(cuts, cuts[1:])):
        check(res[0], I64, k[lo:hi], np.ones(hi - lo, bool), "before the failing batch")
    with pytest.raises(ExecutionError) as x:
        engine().filter_project(None, [prog], parts[2], FL)
    assert (x.value.kind, x.value.message) == ("ArrowError(DivideByZero)", "DivideByZero")
    assert x.value.order_key == err.order_key


def test_a_fallible_child_gives_nulls_with_empty_slots():
    n = 1000
    r = np.random.default_rng(9)
    x = r.random(n) * 6e9 - 3e9  # about a third outside Int32
    x[::50] = np.nan
    schema = Schema([Field("x", F64, True)])
    batch = RecordBatch(schema, [Array.from_numpy(F64, x, r.random(n) > 0.1)])
    child = Cast(Column(0), I32)
    (ref,) = [a for _, a in oracle_filter_project(schema, batch, None, [child], FL & ~TO_UTF8)]
    assert 0 < ref.null_count < n
    prog = compile_scalar_expr(None, Cast(child, U8), schema, FL)
    (got,) = engine().filter_project(None, [prog], batch.to(engine().device), FL)
    check(got, I32, ref.numpy_values(), ref.valid_mask(), "fallible child")


def test_the_host_forms_refuse_a_marked_projection():
    # only filter_project / filter_project_batches format: the host forms would hand back the child's column
    schema, batch = table(100, 84)
    prog = compile_scalar_expr(None, Cast(Column(0), U8), schema, FL)
    refused = ("NotImplemented", "CAST to Utf8 in")
    for call in (lambda: engine().filter_project_host(None, [prog], batch, FL),
                 lambda: engine().filter_project_host_batches(None, [prog], [batch, batch], FL),
                 lambda: engine().filter_project_host_batches_async(None, [prog], [batch, batch], FL)):
        with pytest.raises(ExecutionError) as e:
            call()
        assert (e.value.kind, e.value.message[:15]) == refused


def test_order_by_the_cast_is_bytewise():
    n = 400
    r = np.random.default_rng(10)
    k = r.permutation(n) + 1  # 1 .. 400: "10" < "100" < "101" < .. < "9"
    schema = Schema([Field("k", I64, True)])
    dev = RecordBatch(schema, [Array.from_numpy(I64, k)]).to(engine().device)

    def run(sql):  # (a MemoryDataSource is read once: a context per query)
        ctx = ExecutionContext(flags=FL | _abi.DFMI_FLAG_EXT_SORT)
        ctx.register_datasource("t", MemoryDataSource(schema, [dev]))
        return [int(v) for b in pull_all(ctx.sql(sql)) for v in b.column(0).cpu().numpy_values()]

    want = sorted((int(v) for v in k), key=lambda v: str(v).encode())[:5]
    assert run("SELECT k FROM t ORDER BY CAST(k AS VARCHAR) LIMIT 5") == want == [1, 10, 100, 101, 102]
    assert run("SELECT k FROM t ORDER BY CAST(k AS VARCHAR) DESC LIMIT 3") == [99, 98, 97]


def test_the_serde_worker():
    schema, batch = table(3000, 83)
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(schema, [batch]))
    plan = SqlToRel(ctx).sql_to_rel(SQL)
    t = pa.ipc.open_stream(serde.run_physical_plan(ctx, serde.to_json(serde.Interactive(plan)))).read_all()
    ref = [a for _, a in oracle_filter_project(schema, batch, PRED, CHILDREN, FL & ~TO_UTF8)]
    assert t.num_rows == ref[0].length and [str(f.type) for f in t.schema] == ["string"] * 3
    want_k = [text(I64, v).decode() if ok else None for v, ok in zip(ref[0].numpy_values(), ref[0].valid_mask())]
    assert t.column(0).to_pylist() == want_k
    assert t.column(1).to_pylist() == [text(F64, v).decode() for v in ref[1].numpy_values()]
    assert t.column(2).to_pylist() == [s.decode() for s in ref[2].numpy_values()]
