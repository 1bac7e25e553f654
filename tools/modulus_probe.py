"""Modulus probe (DESIGN.md §6 "Modulus"): what `%` in a predicate costs, and
whether the literal-divisor path (a multiply-high by a host-computed
reciprocal, jit_skeleton.hip irem_lit) beats the general software remainder
(irem) for `col % literal`. One Int64 column k uniform in [0, 2^40) and one
Int32 column k32 uniform in [0, 2^31) read as CAST(k32 AS Int64), 1e8 rows by
default, one device batch. Per column:

  lit      SELECT k FROM t WHERE k % 10 = 3        the default (literal) path
  general  the same with DFMI_DIAG=1 DFMI_REM_LITERAL=0 (the general path forced)
  col      SELECT k FROM t WHERE k % j = 3         j an Int64 column in [7, 13]
  floor    SELECT k FROM t WHERE k = 3             (selects nothing)
  floor10  SELECT k FROM t WHERE k < max / 10      (selects the same 10% as lit)

The knob is read when the library loads, so every measurement runs in a child
process; the parent alternates literal and general children (--pairs pairs, on
the same box) and counts the pairs in which the literal path is not slower.
Each case is the median of --iters HIP-event timings after 0.5 s of warm-up
calls (the clock ramp, DESIGN.md §4 "Utf8 gather (round 5)").

    python tools/modulus_probe.py [--rows N] [--iters K] [--pairs P] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12  # B/s


def timed(fn, iters, warm_s=0.5):
    """Median milliseconds of `iters` HIP-event timings of fn(), after warm_s seconds of calls."""
    import torch
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


def child(mode, n, iters):
    import torch

    from datafusion_amd import _abi
    from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
    from datafusion_amd.execution.engine import engine
    from datafusion_amd.execution.expression import compile_scalar_expr
    from datafusion_amd.logicalplan import BinaryExpr, Cast, Column, DataType, Int64, Literal, Operator

    flags = _abi.DFMI_FLAG_EXT_MODULUS | _abi.DFMI_FLAG_EXT_GATHER_ALL | _abi.DFMI_FLAG_EXT_CAST
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    k = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g)
    j = torch.randint(7, 14, (n,), dtype=torch.int64, device=dev, generator=g)
    k32 = torch.randint(0, (1 << 31) - 1, (n,), dtype=torch.int32, device=dev, generator=g)
    schema = Schema([Field("k", DataType.Int64, False), Field("j", DataType.Int64, False), Field("k32", DataType.Int32, False)])
    batch = RecordBatch(schema, [Array(DataType.Int64, n, k.view(torch.uint8)), Array(DataType.Int64, n, j.view(torch.uint8)),
                                 Array(DataType.Int32, n, k32.view(torch.uint8))])
    eng = engine(dev)
    i64 = lambda v: Literal(Int64(v))
    mod = lambda l, r: BinaryExpr(l, Operator.Modulus, r)
    eq3 = lambda e: BinaryExpr(e, Operator.Eq, i64(3))
    cols = {"int64": (Column(0), 0, 8, 1 << 40), "int32_cast": (Cast(Column(2), DataType.Int64), 2, 4, (1 << 31) - 1)}
    for cname, (kx, out_col, width, top) in cols.items():
        cases = {"lit": eq3(mod(kx, i64(10)))}
        if mode == "literal":  # the cases the knob does not touch run once per pair, in this child
            cases.update({"col": eq3(mod(kx, Column(1))), "floor": eq3(kx),
                          "floor10": BinaryExpr(kx, Operator.Lt, i64(top // 10))})
        proj = [compile_scalar_expr(None, Column(out_col), schema, flags)]
        for case, e in cases.items():
            pred = compile_scalar_expr(None, e, schema, flags)
            out = {}

            def call():
                out["cols"] = eng.filter_project(pred, proj, batch, flags)

            med, ms = timed(call, iters)
            m = out["cols"][0].length
            by = n * (width + (8 if case == "col" else 0)) + m * width
            name = "general" if (case == "lit" and mode == "general") else case
            print(json.dumps({"column": cname, "case": name, "rows": n, "out_rows": m,
                              "kernel": _abi.lib().dfmi_last_kernel_name(eng.ctx).decode(), "call_ms": round(med, 4),
                              "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "rows_per_s": n / (med * 1e-3),
                              "frac_of_8TBs": round(by / (med * 1e-3) / PEAK, 4)}), flush=True)
            if case == "lit":  # the selection itself, against torch
                want = int(((k if cname == "int64" else k32.to(torch.int64)) % 10 == 3).sum().item())
                assert m == want, (cname, mode, m, want)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["literal", "general"])
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.rows, max(10, args.iters))
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    runs = {"literal": [], "general": []}
    for pair in range(max(3, args.pairs)):
        for mode in ("literal", "general"):
            env = {k: v for k, v in os.environ.items() if k != "DFMI_REM_LITERAL"}
            if mode == "general":
                env.update(DFMI_DIAG="1", DFMI_REM_LITERAL="0")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--rows", str(args.rows),
                                "--iters", str(args.iters)], capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return 1  # (nothing more is started after a failed child)
            recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
            for rec in recs:
                rec["pair"] = pair
                emit(rec)
            runs[mode].append(recs)
    ok = True
    for cname in ("int64", "int32_cast"):
        pick = lambda recs, case: next(x for x in recs if x["column"] == cname and x["case"] == case)
        lit = [pick(r, "lit") for r in runs["literal"]]
        gen = [pick(r, "general") for r in runs["general"]]
        ok = ok and all(a["kernel"] != b["kernel"] and a["out_rows"] == b["out_rows"] for a, b in zip(lit, gen))
        wins = sum(a["call_ms"] <= b["call_ms"] for a, b in zip(lit, gen))
        med = lambda case: statistics.median(pick(r, case)["call_ms"] for r in runs["literal"])
        emit({"case": "summary", "column": cname, "pairs": len(lit),
              "literal_ms": [a["call_ms"] for a in lit], "general_ms": [b["call_ms"] for b in gen],
              "pairs_literal_not_slower": wins, "literal_is_default": wins >= 3,
              "median_ms": {"lit": med("lit"), "general": statistics.median(b["call_ms"] for b in gen),
                            "col": med("col"), "floor": med("floor"), "floor10": med("floor10")}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
