"""What CAST to Utf8 costs on the device (DESIGN.md §6 "CAST to Utf8").

Per type, one device column: the time of dfmi_format_utf8_batches into a
pre-allocated exact-size buffer (measure + scan + write: one call), next to a
device-to-device copy of the same input + output bytes on the same box, timed
in alternating pairs -- that copy is the bound, and time / copy the figure.
Floats also report the measure-only call (what a Float64 caller pays first)
and the share of rows on each digit path (DFMI_DIAG=1). Each variant is warmed
for 0.5 s; medians of `--reps` HIP-event timings. One JSON line per case on
stdout (kept under profiles/cast_to_utf8/).

    python tools/format_probe.py [--rows 100000000] [--float-rows 50000000] [--reps 5] [--types Float64]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DFMI_DIAG", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from datafusion_amd import _abi
from datafusion_amd.arrow import Array
from datafusion_amd.execution.engine import column_struct, engine
from datafusion_amd.logicalplan import DataType

FLAGS = _abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_CAST_UTF8
# the tensor type that holds a column's bits (an unsigned column: the signed type of its width, values wrapped)
TORCH = {DataType.Int8: torch.int8, DataType.Int16: torch.int16, DataType.Int32: torch.int32,
         DataType.Int64: torch.int64, DataType.UInt8: torch.uint8, DataType.UInt16: torch.int16,
         DataType.UInt32: torch.int32, DataType.UInt64: torch.int64, DataType.Float32: torch.float32,
         DataType.Float64: torch.float64}


def column(t, kind, n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    if t == DataType.Boolean:
        bits = torch.randint(0, 256, ((n + 63) // 64 * 8,), dtype=torch.uint8, device=dev, generator=g)
        return Array(t, n, bits)
    if kind == "prices":  # two decimals, below 1e5: d / 100 correctly rounded -- a tensor divisor, since
        # torch divides by a Python scalar as a multiply by its reciprocal, which is another double
        # (16 or 17 digits) for one value in eight
        d = torch.randint(0, 10 ** 7, (n,), device=dev, generator=g).to(torch.float64)
        v = torch.div(d, torch.full_like(d, 100.0)).to(TORCH[t])
    elif kind == "random":  # 17 (9) significant digits, one decade
        v = (torch.rand((n,), dtype=torch.float64, device=dev, generator=g) * 1000.0).to(TORCH[t])
    elif kind == "integral":
        v = torch.randint(0, 10 ** 6, (n,), device=dev, generator=g).to(TORCH[t])
    else:  # integers: the type's range, at most 1e12 in magnitude
        lo, hi = {DataType.Int8: (-128, 128), DataType.UInt8: (0, 256), DataType.Int16: (-32768, 32768),
                  DataType.Int32: (-2 ** 31, 2 ** 31), DataType.Int64: (-10 ** 12, 10 ** 12),
                  DataType.UInt16: (0, 2 ** 16), DataType.UInt32: (0, 2 ** 32), DataType.UInt64: (0, 10 ** 12)}[t]
        v = torch.randint(lo, hi, (n,), device=dev, generator=g).to(TORCH[t])
    return Array(t, n, v.view(torch.uint8))


class Call:
    def __init__(self, eng, a, data_bytes):
        self.eng, self.a = eng, a
        self.col = (_abi.dfmi_column * 1)(column_struct(a))
        self.rows = (C.c_int64 * 1)(a.length)
        self.out = (_abi.dfmi_out_column * 1)()
        self.lens = (C.c_int64 * 1)()
        self.offsets = torch.empty(a.length + 1, dtype=torch.int32, device=eng.device)
        self.out[0].offsets = self.offsets.data_ptr()
        self.data = None
        if data_bytes is not None:
            self.data = torch.empty(max(8, data_bytes), dtype=torch.uint8, device=eng.device)
            self.out[0].data, self.out[0].data_capacity = self.data.data_ptr(), data_bytes

    def __call__(self):
        err = _abi.dfmi_error()
        rc = _abi.lib().dfmi_format_utf8_batches(self.eng.ctx, self.col, self.rows, 1, self.out, self.lens, FLAGS,
                                                 C.byref(err))
        if rc != _abi.DFMI_OK:
            raise RuntimeError(err.message.decode())
        return self.lens[0]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--float-rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--types", default="", help="comma-separated type names (default: all)")
    args = ap.parse_args()
    eng = engine("cuda:0")
    L = _abi.lib()
    L.dfmi_context_set_stream(eng.ctx, C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream))
    L.dfmi_internal_format_paths.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    cases = [(DataType.Boolean, "values"), (DataType.Int8, "values"), (DataType.UInt8, "values"),
             (DataType.Int16, "values"), (DataType.UInt16, "values"), (DataType.Int32, "values"),
             (DataType.UInt32, "values"), (DataType.Int64, "values"), (DataType.UInt64, "values"),
             (DataType.Float32, "prices"), (DataType.Float32, "random"), (DataType.Float64, "integral"),
             (DataType.Float64, "prices"), (DataType.Float64, "random")]
    only = {x for x in args.types.split(",") if x}
    for t, kind in cases:
        if only and t.name not in only:
            continue
        isf = t in (DataType.Float32, DataType.Float64)
        n = args.float_rows if isf else args.rows
        a = column(t, kind, n, eng.device)
        measure = Call(eng, a, None)
        need = measure()
        paths = (C.c_uint64 * 4)()
        L.dfmi_internal_format_paths(eng.ctx, paths)
        full = Call(eng, a, need)
        in_bytes = a.values.numel()
        moved = in_bytes + need + 4 * (n + 1)
        src = torch.empty(moved, dtype=torch.uint8, device=eng.device)
        dst = torch.empty(moved, dtype=torch.uint8, device=eng.device)
        copy = lambda: dst.copy_(src)
        warm(full)
        warm(copy)
        tf, tc = [], []
        for _ in range(args.reps):  # alternating pairs
            tf.append(timed(full))
            tc.append(timed(copy))
        line = {"type": t.name, "kind": kind, "rows": n, "out_bytes": int(need), "bytes_per_row": round(need / n, 2),
                "format_ms": round(statistics.median(tf), 3), "copy_ms": round(statistics.median(tc), 3),
                "ratio": round(statistics.median(tf) / statistics.median(tc), 2),
                "pairs_won_by_copy": sum(c < f for f, c in zip(tf, tc))}
        if isf:
            warm(measure)
            line["measure_only_ms"] = round(statistics.median([timed(measure) for _ in range(args.reps)]), 3)
            line["paths"] = {"integer": int(paths[1]), "decimal": int(paths[2]), "exact": int(paths[3])}
        print(json.dumps(line), flush=True)
        del src, dst, full, measure, a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
