"""What CSV output costs on the device (DESIGN.md §6 "CSV output").

Two schemas at `--rows` rows, one device batch each:
  numeric  five columns -- Int32, Int64, UInt16, Float64 prices (two decimals), Float64 integral;
  c3       the C3 shape of bench.py: Utf8 s (the 1000-word dictionary) + Float64 v (random, 10 % nulls).
Per schema: the device time of each phase of one dfmi_csv_encode_batches into a
pre-allocated exact-size buffer (quote scan, measure, scan, write: HIP events
the library records under DFMI_DIAG=1), the whole call, the measure-only call,
and the device-to-host copy of the stream into pinned memory. For the numeric
schema also dfmi_format_utf8_batches over the same five columns in the same
process -- the same digit work, column-major: the yardstick, timed in
alternating pairs with the encode -- and for both pyarrow.csv.write_csv of the
same batch on the host, for scale. Each variant is warmed for 0.5 s; medians of
`--reps` timings. One JSON line per schema on stdout (kept under
profiles/csv_write/).

    python tools/csv_write_probe.py [--rows 10000000] [--reps 5] [--schemas numeric,c3] [--no-host]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DFMI_DIAG", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution.engine import column_struct, engine
from datafusion_amd.logicalplan import DataType

ON = _abi.DFMI_FLAG_EXT_CSV_WRITE
CAST = _abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_CAST_UTF8
PHASES = ("quote_scan", "measure", "scan", "write")


def numeric_batch(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    d = torch.randint(0, 10 ** 7, (n,), device=dev, generator=g).to(torch.float64)
    cols = [
        (DataType.Int32, torch.randint(-2 ** 31, 2 ** 31, (n,), device=dev, generator=g).to(torch.int32)),
        (DataType.Int64, torch.randint(-10 ** 12, 10 ** 12, (n,), device=dev, generator=g)),
        (DataType.UInt16, torch.randint(0, 2 ** 16, (n,), device=dev, generator=g).to(torch.int16)),
        (DataType.Float64, torch.div(d, torch.full_like(d, 100.0))),  # (a tensor divisor: the correctly rounded d / 100)
        (DataType.Float64, torch.randint(0, 10 ** 6, (n,), device=dev, generator=g).to(torch.float64)),
    ]
    schema = Schema([Field("c%d" % i, t, False) for i, (t, _) in enumerate(cols)])
    return RecordBatch(schema, [Array(t, n, v.view(torch.uint8)) for t, v in cols])


def c3_batch(n, dev):
    import bench
    words = bench._utf8_dictionary(bench.SEED)
    dict_bytes = torch.tensor(np.frombuffer(b"".join(words), dtype=np.uint8), device=dev)
    dict_len = torch.tensor([len(w) for w in words], dtype=torch.int64, device=dev)
    dict_off = torch.cumsum(dict_len, 0) - dict_len
    g = torch.Generator(device=dev)
    g.manual_seed(bench.SEED + 1000)
    cols, _ = bench._c3_batch(dev, g, n, dict_bytes, dict_off, dict_len)
    return RecordBatch(Schema([Field("s", DataType.Utf8, False), Field("v", DataType.Float64, True)]), cols)


class Encode:
    def __init__(self, eng, batch, capacity):
        self.eng = eng
        self.carr = (_abi.dfmi_column * len(batch.columns))(*[column_struct(a) for a in batch.columns])
        self.cb = (_abi.dfmi_batch * 1)()
        self.cb[0].num_columns, self.cb[0].num_rows, self.cb[0].columns = len(batch.columns), batch.num_rows(), self.carr
        self.need = C.c_int64(0)
        self.data = torch.empty(max(8, capacity), dtype=torch.uint8, device=eng.device) if capacity is not None else None
        self.capacity = capacity or 0

    def __call__(self):
        err = _abi.dfmi_error()
        rc = _abi.lib().dfmi_csv_encode_batches(self.eng.ctx, self.cb, 1, self.data.data_ptr() if self.data is not None
                                                else None, self.capacity, C.byref(self.need), None, ON, C.byref(err))
        if rc != _abi.DFMI_OK:
            raise RuntimeError(err.message.decode())
        return self.need.value

    def phases(self):
        out = (C.c_double * 4)()
        _abi.lib().dfmi_internal_csv_phases(self.eng.ctx, out)
        return list(out)


class Format:
    """dfmi_format_utf8_batches over the batch's columns into exact-size buffers."""

    def __init__(self, eng, batch):
        self.eng = eng
        n = len(batch.columns)
        self.n = n
        self.cols = (_abi.dfmi_column * n)(*[column_struct(a) for a in batch.columns])
        self.rows = (C.c_int64 * n)(*[a.length for a in batch.columns])
        self.out = (_abi.dfmi_out_column * n)()
        self.lens = (C.c_int64 * n)()
        self.keep = []
        for i, a in enumerate(batch.columns):
            offs = torch.empty(a.length + 1, dtype=torch.int32, device=eng.device)
            self.keep.append(offs)
            self.out[i].offsets = offs.data_ptr()
        self()  # measure
        for i in range(n):
            d = torch.empty(max(8, self.lens[i]), dtype=torch.uint8, device=eng.device)
            self.keep.append(d)
            self.out[i].data, self.out[i].data_capacity = d.data_ptr(), self.lens[i]
        self.bytes = sum(self.lens[i] for i in range(n))

    def __call__(self):
        err = _abi.dfmi_error()
        rc = _abi.lib().dfmi_format_utf8_batches(self.eng.ctx, self.cols, self.rows, self.n, self.out, self.lens, CAST,
                                                 C.byref(err))
        if rc != _abi.DFMI_OK:
            raise RuntimeError(err.message.decode())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def warm(fn, seconds=0.5):
    t0 = time.time()
    while time.time() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def med(xs):
    return round(statistics.median(xs), 3)


def host_write_ms(batch, reps):
    """pyarrow.csv.write_csv of the same batch on the host, into memory."""
    import pyarrow as pa
    import pyarrow.csv as pacsv

    from datafusion_amd import serde
    pb = pa.record_batch([serde.to_arrow_array(c) for c in batch.columns], schema=serde._pa_schema(batch.schema))
    ts = []
    for _ in range(reps):
        sink = io.BytesIO()
        t0 = time.perf_counter()
        pacsv.write_csv(pb, sink)
        ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts), sink.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--schemas", default="numeric,c3")
    ap.add_argument("--no-host", action="store_true", help="skip pyarrow.csv.write_csv")
    args = ap.parse_args()
    eng = engine("cuda:0")
    L = _abi.lib()
    L.dfmi_context_set_stream(eng.ctx, C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    L.dfmi_internal_csv_phases.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    for name in [s for s in args.schemas.split(",") if s]:
        batch = numeric_batch(args.rows, eng.device) if name == "numeric" else c3_batch(args.rows, eng.device)
        measure = Encode(eng, batch, None)
        need = measure()
        full = Encode(eng, batch, need)
        warm(full)
        fmt = Format(eng, batch) if name == "numeric" else None
        if fmt:
            warm(fmt)
        te, tf, ph = [], [], []
        for _ in range(args.reps):  # alternating pairs
            te.append(timed(full))
            ph.append(full.phases())
            if fmt:
                tf.append(timed(fmt))
        warm(measure)
        tm = [timed(measure) for _ in range(args.reps)]
        pinned = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        copy = lambda: pinned.copy_(full.data[:need], non_blocking=True)
        warm(copy)
        tc = [timed(copy) for _ in range(args.reps)]
        line = {"schema": name, "rows": args.rows, "out_bytes": int(need), "bytes_per_row": round(need / args.rows, 2),
                "encode_ms": med(te), "measure_only_ms": med(tm), "d2h_ms": med(tc),
                "phases_ms": {p: med([x[i] for x in ph]) for i, p in enumerate(PHASES)}}
        line["encode_gbps_out"] = round(need / med(te) / 1e6, 2)
        if fmt:
            line["format_utf8_ms"] = med(tf)
            line["format_utf8_bytes"] = int(fmt.bytes)
            line["encode_over_format_utf8"] = round(statistics.median(te) / statistics.median(tf), 2)
            line["pairs_won_by_format_utf8"] = sum(f < e for e, f in zip(te, tf))
        if not args.no_host:
            ms, nbytes = host_write_ms(batch, max(1, min(3, args.reps)))
            line["pyarrow_write_csv_ms"], line["pyarrow_bytes"] = ms, nbytes
        print(json.dumps(line), flush=True)
        del batch, full, measure, fmt, pinned
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
