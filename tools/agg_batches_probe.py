#!/usr/bin/env python3
"""The aggregate pull loop over 1024-row HOST batches through AggregateRelation:
2^22 rows as 4,096 batches, (i) a Q6-style SUM(p * d) behind a three-column
predicate, (ii) SUM(v), COUNT(v) GROUP BY k over 10,000 Int64 keys -- per query
(a) coalesce=1 (one dfmi_aggregate_batch per pull), (b) coalesce=256
(dfmi_aggregate_host_batches) and (c) the oracle on one core over the same
batches; 0.5 s of warm-up, then the median of RUNS runs.
Gate: (b) <= (a) / 4 for both queries (exit status 1 otherwise).
usage: tools/agg_batches_probe.py [nbatches] [runs]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema  # noqa: E402
from datafusion_amd.execution import ExecutionContext, MemoryDataSource  # noqa: E402
from datafusion_amd.logicalplan import DataType  # noqa: E402
from datafusion_amd.sqlplanner import SqlToRel  # noqa: E402

FL = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_GATHER_ALL
M = 1024


def timed_runs(fn, runs):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # warm-up: kernels compiled, pinned staging grown
        fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def run_sql(schema, batches, sql, coalesce):
    ctx = ExecutionContext(flags=FL, coalesce=coalesce)
    ctx.register_datasource("t", MemoryDataSource(schema, batches))
    rel = ctx.sql(sql)
    out = rel.next()
    return [c.cpu().numpy_values().tobytes() for c in out.columns]


def oracle_run(schema, whole, sql):
    from oracle_ffi import oracle_aggregate, oracle_aggregate_grouped_multi
    ctx = ExecutionContext(flags=FL)
    ctx.register_datasource("t", MemoryDataSource(schema, []))
    plan = SqlToRel(ctx).sql_to_rel(sql)
    pred = plan.input.expr if hasattr(plan.input, "expr") else None
    if plan.group_expr:
        return lambda: oracle_aggregate_grouped_multi(schema, whole, pred, list(plan.group_expr), list(plan.aggr_expr), FL, M)
    return lambda: oracle_aggregate(schema, whole, pred, list(plan.aggr_expr), FL, M)


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    torch.cuda.set_device(0)
    n = nb * M
    rng = np.random.default_rng(7)
    queries = []
    s1 = Schema([Field(c, DataType.Float64, False) for c in ("q", "p", "d", "s")])
    c1 = [rng.random(n) * 50, rng.random(n) * 1e5, rng.integers(0, 11, n) / 100.0, rng.random(n)]
    queries.append(("q6", s1, [Array.from_numpy(DataType.Float64, c) for c in c1],
                    "SELECT SUM(p * d) FROM t WHERE s >= 0.3 AND s < 0.5 AND d >= 0.05 AND d <= 0.07 AND q < 24", 3e8))
    s2 = Schema([Field("k", DataType.Int64, False), Field("v", DataType.Float64, False)])
    queries.append(("group_by_10k", s2, [Array.from_numpy(DataType.Int64, rng.integers(0, 10_000, n) * 1_000_003),
                                         Array.from_numpy(DataType.Float64, rng.standard_normal(n))],
                    "SELECT k, SUM(v), COUNT(v) FROM t GROUP BY k", 1e8))
    ok = True
    for name, schema, cols, sql, aim in queries:
        whole = RecordBatch(schema, cols)
        batches = [RecordBatch(schema, [_view(a, i) for a in cols]) for i in range(nb)]
        ref = run_sql(schema, batches, sql, 1)
        assert run_sql(schema, batches, sql, 256) == ref, "coalesce=256 differs from coalesce=1"
        ta = timed_runs(lambda: run_sql(schema, batches, sql, 1), runs)
        tb = timed_runs(lambda: run_sql(schema, batches, sql, 256), runs)
        orc = oracle_run(schema, whole, sql)
        tc = statistics.median([_t(orc) for _ in range(max(3, runs))])
        ratio = ta / tb
        gate = tb <= ta / 4
        ok = ok and gate
        print("%s: %d rows in %d batches of %d" % (name, n, nb, M))
        print("  (a) coalesce=1   %9.2f ms  %7.2f us/batch  %.3g rows/s" % (ta * 1e3, ta / nb * 1e6, n / ta))
        print("  (b) coalesce=256 %9.2f ms  %7.2f us/batch  %.3g rows/s  (aim >= %.0e rows/s: %s)" % (
            tb * 1e3, tb / nb * 1e6, n / tb, aim, "met" if n / tb >= aim else "not met"))
        print("  (c) oracle, 1 core %7.2f ms  %7.2f us/batch  %.3g rows/s" % (tc * 1e3, tc / nb * 1e6, n / tc))
        print("  (a) / (b) = %.2f  gate (b) <= (a) / 4: %s" % (ratio, "PASS" if gate else "FAIL"), flush=True)
    return 0 if ok else 1


def _view(a, i):
    w = a.data_type.width
    return Array(a.data_type, M, a.values[i * M * w:(i + 1) * M * w])


def _t(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


if __name__ == "__main__":
    sys.exit(main())
