"""GPU tests of CSV output (DFMI_FLAG_EXT_CSV_WRITE): the stream's bytes and
batch_ends compared exactly.

The expected bytes always come from the Python restatement of the contract
(tests/csv_write_cases.py, pinned without a GPU by tests/test_csv_write_cpu.py)
and never from the device."""
import ctypes as C
import os

import numpy as np
import pyarrow as pa
import pytest
import torch

from csv_write_cases import (BOOL, F64, QUOTING, TYPES, UTF8, all_types_batch, assert_reads_back, encode_batch,
                             encode_batches, header, make_array, one_type_batch, some_nulls, values)
from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution import ExecutionContext, MemoryDataSource, NativeCsvDataSource
from datafusion_amd.execution.engine import column_struct, engine
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.logicalplan import DataType
from datafusion_amd.sqlplanner import SqlToRel
from golden_cases import CITIES, GOLDEN, all_types_typed, load_batch

pytestmark = pytest.mark.gpu

ON = getattr(_abi, "DFMI_FLAG_EXT_CSV_WRITE", 0x2000)
T = 256       # the kernels' tile rows (csrc/csv_write.h kTileRows)
IMAGE = 4096  # ... and the LDS image of one 64-row slice (kImageBytes)
I32, I64 = DataType.Int32, DataType.Int64


def dev(b: RecordBatch) -> RecordBatch:
    return b.to(engine().device)


def encode(batches, flags=ON):
    data, ends = engine().csv_encode_batches(batches, flags)
    return bytes(data.cpu().numpy()), ends


def check(batches, what=""):
    """The device's stream and batch_ends over `batches` are the restatement's."""
    got, ends = encode([dev(b) for b in batches])
    want, want_ends = encode_batches(batches)
    assert ends == want_ends, (what, ends, want_ends)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        i = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        raise AssertionError("%s: record %d: got %r want %r" % (what, i, g[i:i + 1], w[i:i + 1]))


def pull_all(rel):
    out = []
    while True:
        b = rel.next()
        if b is None:
            return out
        out.append(b)


# ------------------------------------------------- 1. every type, every row count
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 1000]


@pytest.mark.parametrize("t", TYPES, ids=[t.name for t in TYPES])
def test_every_type_alone_and_row_count(t):
    batches = [one_type_batch(t, n, 100 + n + 7 * nulls, bool(nulls)) for n in SIZES for nulls in (0, 1)]
    for b in batches:
        check([b], "%s n=%d nulls=%d" % (t.name, b.num_rows(), b.columns[0].null_count))
    check(batches, "%s, every size in one call" % t.name)


def test_all_thirteen_columns():
    check([all_types_batch(1000, 5)], "thirteen columns")


# ------------------------------------------------- 2. quoting
def one_column(strings) -> RecordBatch:
    return RecordBatch(Schema([Field("s", UTF8, True)]), [Array.from_strings(strings)])


def middle_column(strings) -> RecordBatch:
    n = len(strings)
    return RecordBatch(Schema([Field("a", I32, True), Field("s", UTF8, True), Field("f", F64, True)]),
                       [make_array(I32, np.arange(n) - 5, np.arange(n) % 3 != 0), Array.from_strings(strings),
                        make_array(F64, np.arange(n) * 0.25 - 3, np.arange(n) % 5 != 0)])


@pytest.mark.parametrize("shape", [one_column, middle_column], ids=["alone", "middle-of-three"])
def test_quoting_corpus(shape):
    check([shape(QUOTING)], "the corpus")
    for s in QUOTING:  # ... and every string as the only row: nothing around it in the column's bytes
        check([shape([s])], repr(s)[:40])


@pytest.mark.parametrize("shape", [one_column, middle_column], ids=["alone", "middle-of-three"])
def test_special_bytes_at_the_edges_of_the_columns_data(shape):
    """A special byte in the first and in the last byte of the column's data -- the edges of the scan's
    16-byte loads -- at every alignment of the end, and of the start once the column is sliced."""
    for total in list(range(1, 40)) + [4096 - 1, 4096, 4096 + 1, 2 * 4096 + 17]:
        body = b"x" * max(0, total - 2)
        first, last = b'"' + body[: len(body) // 2], body[len(body) // 2:] + b","
        strings = [first, last] if total > 1 else [b","]
        check([shape(strings)], "%d data bytes" % total)
    for off in range(1, 20):  # rows before a slice hold special bytes that belong to no row of it
        strings = [b'",\n\r'] * off + [b"\rhead", b"mid", b"tail\n"] + [b",,,,"] * 3
        host = shape(strings)
        want = encode_batch(RecordBatch(host.schema, [c.slice(off, 3) for c in host.columns]))
        full = dev(host)
        cut = RecordBatch(full.schema, [c.slice(off, 3) for c in full.columns])
        assert encode([cut])[0] == want, off


# ------------------------------------------------- 3. the LDS image next to the per-lane path
def test_image_overflow_next_to_no_overflow():
    """One tile: slices 0 and 2 of short rows (staged), slice 1 of Float64 subnormals (327 bytes each) and slice 3
    of long strings (spans past the image: stored per lane); then a second tile of short rows."""
    n = 2 * T
    f = np.arange(n) * 0.5
    f[64:128] = -np.finfo(np.float64).smallest_subnormal
    s = [b"r%d" % i for i in range(n)]
    for i in range(192, 256):
        s[i] = (b"long,%d," % i) + b"y" * (100 + i % 7)
    b = RecordBatch(Schema([Field("f", F64, True), Field("s", UTF8, True)]),
                    [make_array(F64, f, np.arange(n) % 11 != 0), Array.from_strings(s)])
    rows = encode_batch(b).split(b"\n")
    assert sum(len(r) + 1 for r in rows[64:128]) > IMAGE and sum(len(r) + 1 for r in rows[192:256]) > IMAGE
    assert sum(len(r) + 1 for r in rows[0:64]) < IMAGE and sum(len(r) + 1 for r in rows[128:192]) < IMAGE
    check([b], "overflow next to none")
    # a slice whose span is exactly the image, one byte less and one more (the alignment's 0..3 bytes included)
    for extra in range(-4, 5):
        lens = [IMAGE // 64 - 1] * 64
        lens[63] += extra
        check([one_column([b"z" * k for k in lens])], "span %+d" % extra)


# ------------------------------------------------- 4. batches, slices, grids
def test_several_batches_in_one_call():
    sizes = [300, 0, 1, 64, 0, 257, 5]
    check([all_types_batch(n, 60 + i) for i, n in enumerate(sizes)], "thirteen columns, seven batches")
    check([one_type_batch(UTF8, n, 80 + i) for i, n in enumerate(sizes)], "Utf8, seven batches")
    check([one_type_batch(I64, 0, 1), one_type_batch(I64, 0, 2)], "only empty batches")
    data, ends = engine().csv_encode_batches([], ON)
    assert data.numel() == 0 and ends == []


@pytest.mark.parametrize("off", [1, 7, 63, 65])
def test_sliced_columns(off):
    n = T + 37
    full = all_types_batch(n + off + 3, 90 + off)
    want = encode_batch(RecordBatch(full.schema, [c.slice(off, n) for c in full.columns]))
    d = dev(full)
    cut = RecordBatch(d.schema, [c.slice(off, n) for c in d.columns])
    assert all(c.offset == off for c in cut.columns)
    got, ends = encode([cut, cut])
    assert got == want + want and ends == [len(want), 2 * len(want)]


def test_past_one_scan_block_and_past_one_grid(monkeypatch):
    n = 70_001
    r = np.random.default_rng(17)
    strings = [b"w%d" % i if i % 97 else b'q"%d,' % i for i in range(n)]
    b = RecordBatch(Schema([Field("i", I64, True), Field("s", UTF8, True), Field("f", F64, True)]),
                    [make_array(I64, r.integers(-10 ** 12, 10 ** 12, n), some_nulls(n, 18, 0.1)),
                     Array.from_strings(strings), make_array(F64, np.arange(n) * 0.125 - 1000.0)])
    want, want_ends = encode_batches([b, b])
    d = dev(b)
    assert (encode([d, d])[0] == want), "one grid"
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_CSV_GRID", "3")
    got, ends = encode([d, d])
    assert ends == want_ends and got == want, "a grid of 3 workgroups"


# ------------------------------------------------- 5. the entry point itself
def raw_call(batches, data, capacity, flags=ON, edit=None, ends=True):
    """dfmi_csv_encode_batches over device batches: (rc, message, data_length, batch_ends)."""
    eng = engine()
    nb = len(batches)
    keep = []
    cb = (_abi.dfmi_batch * max(1, nb))()
    for i, b in enumerate(batches):
        carr = (_abi.dfmi_column * max(1, len(b.columns)))(*[column_struct(a) for a in b.columns])
        keep.append(carr)
        cb[i].num_columns, cb[i].num_rows, cb[i].columns = len(b.columns), b.num_rows(), carr
    if edit:
        edit(cb)
    need, err = C.c_int64(-1), _abi.dfmi_error()
    e = (C.c_int64 * max(1, nb))(*([-1] * max(1, nb)))
    rc = _abi.lib().dfmi_csv_encode_batches(eng.ctx, cb, nb, data, capacity, C.byref(need), e if ends else None, flags,
                                           C.byref(err))
    return rc, err.message.decode(), need.value, list(e)[:nb]


def test_measure_then_exact_write_and_one_byte_short():
    batches = [dev(all_types_batch(700, 21)), dev(all_types_batch(0, 22)), dev(all_types_batch(90, 23))]
    want, want_ends = encode_batches(batches)
    rc, msg, need, ends = raw_call(batches, None, 0)  # measure only
    assert (rc, need, ends) == (_abi.DFMI_OK, len(want), want_ends), msg
    buf = torch.full((need + 64,), 0xAA, dtype=torch.uint8, device=engine().device)
    rc, msg, need2, ends = raw_call(batches, C.c_void_p(buf.data_ptr()), need)
    assert (rc, need2, ends) == (_abi.DFMI_OK, need, want_ends), msg
    host = bytes(buf.cpu().numpy())
    assert host[:need] == want and host[need:] == b"\xaa" * 64  # nothing past the stream
    buf.fill_(0xAA)
    rc, msg, need3, ends = raw_call(batches, C.c_void_p(buf.data_ptr()), need - 1, ends=False)
    assert rc == _abi.DFMI_ERR_CAPACITY and need3 == need, msg
    assert bytes(buf.cpu().numpy()) == b"\xaa" * (need + 64)  # no byte written


def test_argument_errors_and_limits():
    a = dev(one_type_batch(I32, 10, 1))
    b = dev(one_type_batch(I64, 10, 2))
    INVALID, NOTIMPL = _abi.DFMI_ERR_INVALID_ARGUMENT, _abi.DFMI_ERR_NOT_IMPLEMENTED
    rc, msg, _, _ = raw_call([a], None, 0, flags=0xffffffff & ~ON)
    assert (rc, msg) == (NOTIMPL, "dfmi_csv_encode_batches needs DFMI_FLAG_EXT_CSV_WRITE")
    assert raw_call([a, b], None, 0)[0] == INVALID  # a type mismatch between batches

    def set_type(cb):
        cb[0].columns[0].type = 13
    assert raw_call([a], None, 0, edit=set_type)[0] == INVALID  # a type outside Boolean .. Utf8

    def set_length(cb):
        cb[0].columns[0].length = 11
    assert raw_call([a], None, 0, edit=set_length)[0] == INVALID

    def negative_rows(cb):
        cb[0].num_rows = -1
        cb[0].columns[0].length = -1
    assert raw_call([a], None, 0, edit=negative_rows)[0] == INVALID

    def null_values(cb):
        cb[0].columns[0].values = None
    assert raw_call([a], None, 0, edit=null_values)[0] == INVALID
    s = dev(one_type_batch(UTF8, 10, 3))

    def null_offsets(cb):
        cb[0].columns[0].offsets = None
    assert raw_call([s], None, 0, edit=null_offsets)[0] == INVALID

    def no_columns(cb):
        cb[0].num_columns = 0
    assert raw_call([a], None, 0, edit=no_columns)[0] == INVALID
    eng = engine()
    err, need = _abi.dfmi_error(), C.c_int64(0)
    assert _abi.lib().dfmi_csv_encode_batches(eng.ctx, None, 1, None, 0, C.byref(need), None, ON, C.byref(err)) == INVALID
    # the program limits: columns, rows (both refused before any buffer is read)
    col = a.columns[0]
    wide = RecordBatch(Schema([Field("c%d" % i, I32, True) for i in range(257)]), [col] * 257)
    rc, msg, _, _ = raw_call([wide], None, 0)
    assert rc == NOTIMPL and msg.startswith("device program limit: ") and "256 columns" in msg
    check([RecordBatch(Schema(wide.schema.fields[:256]), [col.cpu()] * 256)], "256 columns")

    def huge(cb):
        cb[0].num_rows = cb[0].columns[0].length = 1 << 31
    rc, msg, _, _ = raw_call([a], None, 0, edit=huge)
    assert rc == NOTIMPL and msg.startswith("device program limit: ") and "rows" in msg


# ------------------------------------------------- 6. write_csv: relations, fixtures, errors, the worker
def read_back(schema, path, has_header=True):
    return pull_all(NativeCsvDataSource(schema, path, has_header=has_header, batch_size=500))


def test_write_csv_round_trip(tmp_path):
    batches = [all_types_batch(n, 30 + i) for i, n in enumerate([400, 0, 1000, 3])]
    schema = batches[0].schema
    for coalesce, device in ((1, True), (256, True), (256, False)):  # host batches go through the upload path
        ctx = ExecutionContext(flags=ON, coalesce=coalesce)
        src = [dev(b) if device else b for b in batches]
        ctx.register_datasource("t", MemoryDataSource(schema, src))
        from datafusion_amd.execution.context import TableScan
        path = str(tmp_path / ("rt_%d_%d.csv" % (coalesce, device)))
        assert ctx.write_csv(TableScan("t", schema), path) == sum(b.num_rows() for b in batches)
        data = open(path, "rb").read()
        assert data == header([f.name for f in schema.fields]) + encode_batches(batches)[0]
        assert_reads_back(batches, read_back(schema, path), "coalesce %d device %s" % (coalesce, device))
    ctx = ExecutionContext(flags=ON)
    ctx.register_datasource("t", MemoryDataSource(schema, [dev(b) for b in batches]))
    path = str(tmp_path / "no_header.csv")
    from datafusion_amd.execution.relation import DataSourceRelation
    ctx.write_csv(DataSourceRelation(ctx.datasources["t"]), path, has_header=False)  # a relation, not a plan
    assert open(path, "rb").read() == encode_batches(batches)[0]
    with pytest.raises(ExecutionError) as e:
        ExecutionContext(flags=0).write_csv(DataSourceRelation(MemoryDataSource(schema, [])), path)
    assert e.value.kind == "NotImplemented"


def test_a_group_at_the_byte_limit_is_halved(tmp_path, monkeypatch):
    """CsvWriter halves a group the encode refuses for its 2^31 bytes; a single batch of that size is the error.
    (The limit itself needs 2 GB of output: here the engine's call is wrapped to refuse more than two batches.)"""
    from datafusion_amd.execution import CsvWriter
    from datafusion_amd.execution.engine import DeviceEngine
    limit = "device program limit: CSV output of 2^31 or more bytes"
    real, calls = DeviceEngine.csv_encode_batches, []

    def refusing(self, batches, flags, most=2):
        calls.append(len(batches))
        if len(batches) > most:
            raise ExecutionError("NotImplemented", limit)
        return real(self, batches, flags)
    monkeypatch.setattr(DeviceEngine, "csv_encode_batches", refusing)
    batches = [all_types_batch(n, 70 + n) for n in (5, 0, 9, 300, 1, 2, 7)]
    path = str(tmp_path / "halved.csv")
    with CsvWriter(path, batches[0].schema, has_header=False) as w:
        assert w.write(batches) == sum(b.num_rows() for b in batches)
    assert open(path, "rb").read() == encode_batches(batches)[0]
    assert calls == [7, 3, 1, 2, 4, 2, 2]  # halves, in order
    monkeypatch.setattr(DeviceEngine, "csv_encode_batches", lambda self, b, f: refusing(self, b, f, most=0))
    with CsvWriter(path, batches[0].schema) as w:
        with pytest.raises(ExecutionError) as e:
            w.write(batches[:1])
    assert (e.value.kind, e.value.message) == ("NotImplemented", limit)
    assert open(path, "rb").read() == header([f.name for f in batches[0].schema.fields])  # the header, no record


AGG = (_abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY | _abi.DFMI_FLAG_EXT_SORT |
       _abi.DFMI_FLAG_EXT_GATHER_ALL)
FIXTURE_QUERIES = [
    ("cities", "SELECT city, lat, lng FROM cities WHERE lat > 52"),
    ("t", "SELECT c0, MIN(c11), MAX(c10), COUNT(c8) FROM t GROUP BY c0"),
    ("t", "SELECT c11, c10, c8, c0 FROM t ORDER BY c10 DESC, c8 LIMIT 20"),
]


@pytest.mark.parametrize("coalesce", [1, 256])
@pytest.mark.parametrize("table,sql", FIXTURE_QUERIES, ids=["where", "group-by", "order-by-limit"])
def test_fixture_queries_end_to_end(table, sql, coalesce, tmp_path):
    if table == "cities":
        schema, name = CITIES, "uk_cities.csv"
    else:
        schema, name = all_types_typed(), "all_types_flat.csv"

    def context():
        ctx = ExecutionContext(flags=ON | AGG, coalesce=coalesce)
        ctx.register_datasource(table, NativeCsvDataSource(schema, os.path.join(GOLDEN, name), has_header=True,
                                                           batch_size=16))
        return ctx
    rel = context().sql(sql)
    batches = pull_all(rel)
    assert sum(b.num_rows() for b in batches) > 1
    want = header([f.name for f in rel.schema().fields]) + encode_batches(batches)[0]
    ctx = context()
    path = str(tmp_path / "out.csv")
    rows = ctx.write_csv(SqlToRel(ctx).sql_to_rel(sql), path)
    assert rows == sum(b.num_rows() for b in batches)
    assert open(path, "rb").read() == want
    assert_reads_back(batches, read_back(rel.schema(), path), sql)


@pytest.mark.parametrize("coalesce", [1, 256])
def test_divide_by_zero_in_a_middle_batch(coalesce, tmp_path):
    schema = Schema([Field("a", I64, False), Field("b", I64, False)])
    batches = []
    for k in range(5):
        b = np.arange(1, 101, dtype=np.int64)
        if k == 2:
            b[40] = 0
        batches.append(RecordBatch(schema, [make_array(I64, np.arange(100) * (k + 1)), make_array(I64, b)]))
    sql = "SELECT a, a / b FROM t"

    def context():
        ctx = ExecutionContext(flags=ON, coalesce=coalesce)
        ctx.register_datasource("t", MemoryDataSource(schema, [dev(b) for b in batches]))
        return ctx
    rel = context().sql(sql)
    good = []
    with pytest.raises(ExecutionError) as alone:
        while True:
            good.append(rel.next())
    assert len(good) == 2 and "DivideByZero" in alone.value.kind
    ctx = context()
    path = str(tmp_path / "out.csv")
    with pytest.raises(ExecutionError) as e:
        ctx.write_csv(SqlToRel(ctx).sql_to_rel(sql), path)
    assert (e.value.kind, e.value.message) == (alone.value.kind, alone.value.message)
    head = header([f.name for f in rel.schema().fields])
    want = head + encode_batches(good)[0]
    data = open(path, "rb").read()
    assert want.startswith(data) and data.startswith(head) and data.endswith(b"\n")
    assert data == want  # every batch the pull loop saw before the error


def test_the_serde_worker_writes_the_file(tmp_path):
    batch = load_batch(CITIES, "uk_cities.csv", has_header=True)
    sql = "SELECT city, lat, lng, lat + lng FROM cities WHERE lat > 51.0 AND lat < 53"

    def context(flags):
        ctx = ExecutionContext(flags=flags)
        ctx.register_datasource("cities", MemoryDataSource(CITIES, [batch]))
        return ctx
    ctx = context(ON)
    plan = SqlToRel(ctx).sql_to_rel(sql)
    rel = context(ON).execute(plan)
    names = [f.name for f in rel.schema().fields]  # the relation's schema: what the header and the stream carry
    batches = pull_all(rel)
    for kind in ("csv", "CSV", "Csv"):
        path = str(tmp_path / ("%s.out" % kind))
        stream = serde.run_physical_plan(context(ON), serde.to_json(serde.Write(plan, path, kind)))
        t = pa.ipc.open_stream(stream).read_all()
        assert t.num_rows == 0 and t.schema.names == names and len(names) == 4
        assert open(path, "rb").read() == header(names) + encode_batches(batches)[0]
    path = str(tmp_path / "none.csv")
    with pytest.raises(ExecutionError) as e:
        serde.run_physical_plan(context(0), serde.to_json(serde.Write(plan, path, "csv")))
    assert (e.value.kind, e.value.message) == ("NotImplemented", "PhysicalPlan::Write in a worker")
    assert not os.path.exists(path)
