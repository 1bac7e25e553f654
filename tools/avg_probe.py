"""AVG probe (DESIGN.md §6 "AVG"): what AVG's finish costs next to SUM's. AVG
accumulates exactly as SUM does (the same kernels and code objects); its only
new device cost is the division in the finish (groupby.hip k_group_round,
avg_round.h). One Int64 key and one Float64 argument, 1e7 rows by default in
one device batch, over 1e4 and over 1e6 distinct keys; on the same build, in
one run, per key count:

  SUM(v) GROUP BY k    accumulate call, then dfmi_agg_state_finish_grouped
  AVG(v) GROUP BY k    accumulate call, then dfmi_agg_state_finish_grouped

SUM's finish is code AVG does not touch, so it stands for the build before
AVG. Each call is timed on the host clock (both calls synchronise before they
return; the finish includes its copy of the results to the host) as the
median of --iters calls after 0.5 s of warm-up calls (the clock ramp). A
finish leaves the table as it is, so it is simply repeated; an accumulate
call is repeated on a reset state.

    python tools/avg_probe.py [--rows N] [--iters K] [--out FILE]
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
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr  # noqa: E402
from datafusion_amd.logicalplan import AggregateFunction, Column, DataType  # noqa: E402

FL = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_AVG | _abi.DFMI_FLAG_EXT_GATHER_ALL


def timed(fn, iters, warm_s=0.5, before=None):
    """Median milliseconds (host clock) of `iters` calls of fn(), each after
    before(), following warm_s seconds of such calls."""
    def once():
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        once()
    ms = [once() for _ in range(iters)]
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, iters = args.rows, max(5, args.iters)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    schema = Schema([Field("k", DataType.Int64, False), Field("v", DataType.Float64, False)])
    v = (torch.rand(n, dtype=torch.float64, device=dev, generator=g) - 0.5) * 1e6
    eng = engine(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    key = compile_scalar_expr(None, Column(0), schema, FL)
    for nkeys in (10_000, 1_000_000):
        k = torch.randint(0, nkeys, (n,), dtype=torch.int64, device=dev, generator=g) * 1_000_003
        batch = RecordBatch(schema, [Array(DataType.Int64, n, k.view(torch.uint8)),
                                     Array(DataType.Float64, n, v.view(torch.uint8))])
        res = {}
        for name in ("SUM", "AVG", "SUM"):  # SUM twice: the spread between two runs of the same code
            a = compile_expr(None, AggregateFunction(name, (Column(1),), DataType.Float64), schema, FL)
            st = eng.grouped_agg_state([key], [a])
            acc, acc_ms = timed(lambda: st.add(None, batch, FL), iters, before=st.reset)
            out = {}

            def finish():
                out["r"] = st.finish()

            fin, fin_ms = timed(finish, iters)
            groups = len(out["r"][0])
            tag = name.lower() + ("_again" if name in res else "")
            res[name] = fin
            emit({"case": tag, "rows": n, "keys": nkeys, "groups": groups, "accumulate_ms": round(acc, 3),
                  "accumulate_min_ms": round(min(acc_ms), 3), "finish_ms": round(fin, 3),
                  "finish_min_ms": round(min(fin_ms), 3), "finish_max_ms": round(max(fin_ms), 3),
                  "finish_ns_per_group": round(fin * 1e6 / max(groups, 1), 1)})
            if name == "AVG":
                res["avg_acc"] = acc
        emit({"case": "summary", "keys": nkeys, "avg_minus_sum_finish_ms": round(res["AVG"] - res["SUM"], 3),
              "avg_finish_over_its_accumulate": round(res["AVG"] / res["avg_acc"], 3)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
