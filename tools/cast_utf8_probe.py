"""CAST-from-Utf8 probe (DESIGN.md §6 "Utf8 casts"): what parsing a string
column on the device costs, next to the same query over a pre-parsed column
(the floor) and next to `s < 'lit'` over the same Utf8 column (which reads the
same offsets and head bytes). One device batch, 1.25e8 rows by default:

  si  decimal renderings of integers, 1 to 19 bytes (a uniform digit count)
  sf  repr() of random doubles (a pool of 1e6 values, drawn at random), in a
      batch of its own of half the rows: at ~20 bytes a row 1.25e8 rows would
      pass the 2^31 bytes that Int32 offsets address
  vi  Int64, vf Float64: si / sf parsed ahead of time;  v  Int64 row numbers

  dense   SELECT CAST(si AS Int64)  | SELECT vi + 1     | SELECT si < '5'
          SELECT CAST(sf AS Float64)| SELECT vf + 1.0   | SELECT sf < '5'
  filter  SELECT v WHERE CAST(si AS Int64) < L at 1 / 50 / 99 % selected
          | SELECT v WHERE vi < L | SELECT v WHERE si < 'lit'

Each case is the median of --iters HIP-event timings after 0.5 s of warm-up
calls (the clock ramp, DESIGN.md §4 "Utf8 gather (round 5)"). The measuring
child runs with DFMI_JIT_VERBOSE=1; the parent reads each kernel's VGPRs and
scratch bytes (hipFuncGetAttribute) from its stderr and adds them to the
kernel's records, with whether an 8-waves/SIMD hint held (at most 64 VGPRs).

    python tools/cast_utf8_probe.py [--rows N] [--iters K] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def integer_strings(n, dev, gen, chunk=12_500_000):
    """(values, offsets, bytes): integers of 1 to 19 digits rendered on the device."""
    import torch
    p10 = torch.tensor([10 ** j for j in range(19)], dtype=torch.int64, device=dev)
    lows = [0] + [10 ** (d - 1) if d > 1 else 0 for d in range(1, 20)]            # by digit count (index 0 unused)
    tops = [0] + [min(10 ** d, 1 << 63) - 1 for d in range(1, 20)]                # 19 digits: up to i64::MAX
    low_t = torch.tensor(lows, dtype=torch.int64, device=dev)
    span_t = torch.tensor([t - l + 1 for l, t in zip(lows, tops)], dtype=torch.float64, device=dev)
    top_t = torch.tensor(tops, dtype=torch.int64, device=dev)
    vals, lens, parts = [], [], []
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        L = torch.randint(1, 20, (m,), device=dev, generator=gen)
        u = torch.rand(m, device=dev, generator=gen, dtype=torch.float64)
        v = torch.minimum(low_t[L] + (u * span_t[L]).to(torch.int64), top_t[L])
        c = torch.arange(19, device=dev).unsqueeze(0)
        j = (L.unsqueeze(1) - 1 - c).clamp_(min=0)
        mat = ((v.unsqueeze(1) // p10[j]) % 10 + 48).to(torch.uint8)
        parts.append(mat[c < L.unsqueeze(1)])
        vals.append(v)
        lens.append(L)
    L = torch.cat(lens)
    offs = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(L, 0).to(torch.int32)
    return torch.cat(vals), offs, torch.cat(parts)


def float_strings(n, dev, gen, pool=1_000_000, chunk=10_000_000):
    """(values, offsets, bytes): repr() of a pool of random doubles, drawn at random."""
    import numpy as np
    import torch
    rng = np.random.default_rng(11)
    pv = rng.standard_normal(pool) * 10.0 ** rng.integers(-8, 9, pool)
    texts = [repr(float(x)).encode() for x in pv]
    pl = torch.tensor([len(t) for t in texts], dtype=torch.int64, device=dev)
    po = torch.zeros(pool + 1, dtype=torch.int64, device=dev)
    po[1:] = torch.cumsum(pl, 0)
    pb = torch.frombuffer(bytearray(b"".join(texts)), dtype=torch.uint8).to(dev)
    pvt = torch.from_numpy(pv).to(dev)
    vals, lens, parts = [], [], []
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        idx = torch.randint(0, pool, (m,), device=dev, generator=gen)
        ln = pl[idx]
        o = torch.cumsum(ln, 0) - ln
        pos = torch.arange(int(ln.sum().item()), device=dev) - torch.repeat_interleave(o, ln) + torch.repeat_interleave(po[idx], ln)
        parts.append(pb[pos])
        vals.append(pvt[idx])
        lens.append(ln)
    L = torch.cat(lens)
    offs = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(L, 0).to(torch.int32)
    return torch.cat(vals), offs, torch.cat(parts)


def child(n, iters):
    import torch

    from datafusion_amd import _abi
    from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
    from datafusion_amd.execution.engine import engine
    from datafusion_amd.execution.expression import compile_scalar_expr
    from datafusion_amd.logicalplan import BinaryExpr, Cast, Column, DataType, Float64, Int64, Literal, Operator, Utf8

    flags = (_abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_CAST_ANY | _abi.DFMI_FLAG_EXT_GATHER_ALL |
             _abi.DFMI_FLAG_EXT_UTF8_COMPARE | _abi.DFMI_FLAG_EXT_UTF8_ORDER)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    vi, oi, bi = integer_strings(n, dev, g)
    nf = n // 2  # (repr() takes ~20 bytes a row: 1.25e8 rows would pass the 2^31 bytes Int32 offsets address)
    vf, of, bf = float_strings(nf, dev, g)
    assert int(oi[-1]) == bi.numel() < (1 << 31) and int(of[-1]) == bf.numel() < (1 << 31)
    v = torch.arange(n, dtype=torch.int64, device=dev)
    U8, I64, F64 = DataType.Utf8, DataType.Int64, DataType.Float64
    # one schema, two batches: the integer strings (n rows) and the float strings (n / 2 rows)
    schema = Schema([Field("s", U8, False), Field("p", I64, False), Field("pf", F64, False), Field("v", I64, False)])
    zeros = lambda m: torch.zeros(8 * m, dtype=torch.uint8, device=dev)
    batch_i = RecordBatch(schema, [Array(U8, n, bi, None, oi), Array(I64, n, vi.view(torch.uint8)), Array(F64, n, zeros(n)),
                                   Array(I64, n, v.view(torch.uint8))])
    batch_f = RecordBatch(schema, [Array(U8, nf, bf, None, of), Array(I64, nf, zeros(nf)), Array(F64, nf, vf.view(torch.uint8)),
                                   Array(I64, nf, v[:nf].view(torch.uint8))])
    eng = engine(dev)
    lt = lambda l, r: BinaryExpr(l, Operator.Lt, r)
    cases = [("dense", "int64", "cast", None, Cast(Column(0), I64)),
             ("dense", "int64", "floor", None, BinaryExpr(Column(1), Operator.Plus, Literal(Int64(1)))),
             ("dense", "int64", "utf8_lt", None, lt(Column(0), Literal(Utf8("5")))),
             ("dense", "float64", "cast", None, Cast(Column(0), F64)),
             ("dense", "float64", "floor", None, BinaryExpr(Column(2), Operator.Plus, Literal(Float64(1.0)))),
             ("dense", "float64", "utf8_lt", None, lt(Column(0), Literal(Utf8("5"))))]
    svi = torch.sort(vi[: min(n, 4_000_000)]).values
    for pct, lit in ((1, "10000000000"), (50, "5"), (99, "99")):
        L = int(svi[int(len(svi) * pct / 100)].item())
        cases += [("filter%d" % pct, "int64", "cast", lt(Cast(Column(0), I64), Literal(Int64(L))), Column(3)),
                  ("filter%d" % pct, "int64", "floor", lt(Column(1), Literal(Int64(L))), Column(3)),
                  ("filter%d" % pct, "int64", "utf8_lt", lt(Column(0), Literal(Utf8(lit))), Column(3))]
    for query, column, case, pred, proj in cases:
        p = compile_scalar_expr(None, pred, schema, flags) if pred is not None else None
        cp = [compile_scalar_expr(None, proj, schema, flags)]
        out = {}
        batch, rows = (batch_f, nf) if column == "float64" else (batch_i, n)

        def call(batch=batch):
            out["cols"] = eng.filter_project(p, cp, batch, flags)

        med, ms = timed(call, iters)
        got = out["cols"][0]
        rec = {"query": query, "column": column, "case": case, "rows": rows, "out_rows": got.length,
               "kernel": _abi.lib().dfmi_last_kernel_name(eng.ctx).decode(), "call_ms": round(med, 4),
               "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "rows_per_s": rows / (med * 1e-3)}
        if case == "cast":  # the values themselves, against the pre-parsed column
            if pred is None:
                want = vi if column == "int64" else vf
                same = torch.equal(got.values[: 8 * rows].view(torch.int64), want.view(torch.int64))
                rec["bits_equal_preparsed"] = bool(same) and got.null_count == 0
                assert rec["bits_equal_preparsed"], (query, column)
        print(json.dumps(rec), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.rows, max(10, args.iters))
    env = dict(os.environ, DFMI_JIT_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rows", str(args.rows), "--iters",
                        str(args.iters)], capture_output=True, text=True, env=env, timeout=1100)
    res = {}
    for m in re.finditer(r"dfmi jit: (\S+) waves_per_eu (\d+): scratch (\d+) B/lane, (\d+) VGPRs", r.stderr):
        res[m.group(1)] = {"waves_per_eu_hint": int(m.group(2)), "scratch_bytes": int(m.group(3)), "vgprs": int(m.group(4))}
    lines = []
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    for rec in recs:
        k = res.get(rec["kernel"])
        if k:
            rec.update(k)
            if k["waves_per_eu_hint"] == 8:
                rec["hint_8_waves_held"] = k["vgprs"] <= 64
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
    # the comparison lines: each cast next to its floor and its Utf8 compare
    by = {(x["query"], x["column"], x["case"]): x for x in recs}
    for (q, c, case), x in by.items():
        if case != "cast" or (q, c, "floor") not in by or (q, c, "utf8_lt") not in by:
            continue
        f, u = by[(q, c, "floor")], by[(q, c, "utf8_lt")]
        lines.append(json.dumps({"case": "summary", "query": q, "column": c, "cast_ms": x["call_ms"], "floor_ms": f["call_ms"],
                                 "utf8_lt_ms": u["call_ms"], "cast_over_floor": round(x["call_ms"] / f["call_ms"], 2),
                                 "cast_over_utf8_lt": round(x["call_ms"] / u["call_ms"], 2),
                                 "out_rows": [x["out_rows"], f["out_rows"], u["out_rows"]]}))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
