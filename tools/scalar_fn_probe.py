"""Scalar function probe (DESIGN.md §6 "Scalar functions"): what a function in
a projection costs. Three Float64 columns in [0, 1), 1e8 rows by default, one
device batch; on the same box, in one run:

  (a)  SELECT sqrt(a * a + b * b) FROM t WHERE c < 0.5   (DFMI_FLAG_EXT_SCALAR_FUNCTIONS)
  (b)  SELECT a * a + b * b FROM t WHERE c < 0.5         (the same query without the sqrt)
  (c)  torch: m = c < 0.5; torch.sqrt(a[m] * a[m] + b[m] * b[m])

Each is timed as the median of --iters HIP-event timings after 0.5 s of
warm-up calls (the clock ramp, DESIGN.md §4 "Utf8 gather (round 5)"); (b) is
timed twice, before and after (a), so the difference (a) - (b) can be read
against the spread between two runs of the same kernel. The byte model per
input row: 8 B of c, 16 B of a and b (half the rows are selected, so every
cache line of both columns is touched), and 8 B written per selected row.

    python tools/scalar_fn_probe.py [--rows N] [--iters K] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema  # noqa: E402
from datafusion_amd.execution.engine import engine  # noqa: E402
from datafusion_amd.execution.expression import compile_scalar_expr  # noqa: E402
from datafusion_amd.logicalplan import (BinaryExpr, Column, DataType, Float64, Literal, Operator,  # noqa: E402
                                        ScalarFunction)

PEAK = 8e12  # B/s
FN = _abi.DFMI_FLAG_EXT_SCALAR_FUNCTIONS


def timed(fn, iters, warm_s=0.5):
    """Median milliseconds of `iters` HIP-event timings of fn(), after warm_s seconds of calls."""
    t0 = time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= warm_s:
            break
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, iters = args.rows, max(10, args.iters)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    a, b, c = (torch.rand(n, dtype=torch.float64, device=dev, generator=g) for _ in range(3))
    schema = Schema([Field(nm, DataType.Float64, False) for nm in "abc"])
    batch = RecordBatch(schema, [Array(DataType.Float64, n, t.view(torch.uint8)) for t in (a, b, c)])
    eng = engine(dev)
    pred = compile_scalar_expr(None, BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5))), schema, FN)
    hyp2 = BinaryExpr(BinaryExpr(Column(0), Operator.Multiply, Column(0)), Operator.Plus,
                      BinaryExpr(Column(1), Operator.Multiply, Column(1)))
    with_fn = [compile_scalar_expr(None, ScalarFunction("sqrt", (hyp2,), DataType.Float64), schema, FN)]
    without = [compile_scalar_expr(None, hyp2, schema, FN)]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def dfmi_case(name, projs):
        out = {}

        def call():
            out["cols"] = eng.filter_project(pred, projs, batch, FN)

        med, ms = timed(call, iters)
        m = out["cols"][0].length
        by = n * (8 + 16) + m * 8
        emit({"case": name, "rows": n, "out_rows": m, "kernel": _abi.lib().dfmi_last_kernel_name(eng.ctx).decode(),
              "call_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
              "rows_per_s": n / (med * 1e-3), "frac_of_8TBs": round(by / (med * 1e-3) / PEAK, 4)})
        return med, out["cols"][0]

    b1, _ = dfmi_case("b_without_sqrt", without)
    a_ms, got = dfmi_case("a_with_sqrt", with_fn)
    b2, _ = dfmi_case("b_without_sqrt_again", without)

    def torch_query():
        m = c < 0.5
        am, bm = a[m], b[m]
        return torch.sqrt(am * am + bm * bm)

    med, ms = timed(torch_query, iters)
    emit({"case": "c_torch_composition", "rows": n, "call_ms": round(med, 3), "min_ms": round(min(ms), 3),
          "max_ms": round(max(ms), 3), "rows_per_s": n / (med * 1e-3)})
    ref = torch_query()
    same = got.length == ref.numel() and bool(torch.equal(got.values[: got.length * 8].view(torch.int64),
                                                          ref.view(torch.int64)))
    emit({"case": "summary", "a_minus_b_ms": round(a_ms - (b1 + b2) / 2, 3), "b_spread_ms": round(abs(b1 - b2), 3),
          "agrees_with_torch": same})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
