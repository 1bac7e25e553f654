"""Utf8 MIN / MAX probe (DESIGN.md §6 "MIN / MAX over Utf8"): what
`MIN(s), MAX(s)` costs next to `COUNT(s)` on the same state shape -- the
nearest query the build before the feature runs: inside the kernels a Utf8
extreme IS a COUNT, and the string passes (csrc/str_extreme.hip: prefix,
candidates, measure, keep, twice -- once per extreme) come on top. One device batch of
--rows rows, ungrouped and grouped by 10,000 Int64 keys, over four string
columns:

  c3        the C3 column of bench.py: a 1,000-word dictionary, 2 to 24 bytes
  one       every row the same string (every row a candidate)
  few       25 distinct strings
  prefix16  100,000 distinct strings sharing a 16-byte prefix (every row
            passes the 8-byte prefix filter: the known worst case)

Each accumulate call on a reset state is timed on the host clock (the call
synchronises before it returns) as the median of --iters calls after 0.5 s of
warm-up calls; COUNT(s) is timed before and after the extremes (the spread of
the same code).

    python tools/minmax_utf8_probe.py [--rows N] [--iters K] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema  # noqa: E402
from datafusion_amd.execution.engine import engine  # noqa: E402
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr  # noqa: E402
from datafusion_amd.logicalplan import AggregateFunction, Column, DataType  # noqa: E402

FL = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY | _abi.DFMI_FLAG_EXT_GATHER_ALL


def timed(fn, iters, warm_s=0.5, before=None):
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


def arena_bytes(handle):
    import ctypes as C
    fn = _abi.lib().dfmi_internal_agg_str_arena_bytes
    fn.argtypes, fn.restype = [C.c_void_p], C.c_longlong
    return fn(handle)


def dictionary(kind):
    rng = np.random.default_rng(3)
    if kind == "c3":  # bench.py _utf8_dictionary
        out = []
        for i in range(1000):
            w = b"w%d" % i
            ln = int(rng.integers(len(w), 25))
            out.append(w + bytes(rng.integers(97, 123, ln - len(w)).astype(np.uint8)))
        return out
    if kind == "one":
        return [b"the-only-string"]
    if kind == "few":
        return [b"word-%02d" % i for i in range(25)]
    return [b"shared-prefix-16-%08d" % i for i in range(100_000)]


def utf8_column(dev, g, n, words):
    """n rows drawn uniformly from `words`, built on the device (bench.py _c3_batch's way)."""
    dict_len = torch.tensor([len(w) for w in words], dtype=torch.int64, device=dev)
    dict_off = torch.zeros(len(words), dtype=torch.int64, device=dev)
    dict_off[1:] = torch.cumsum(dict_len, 0)[:-1]
    dict_bytes = torch.frombuffer(bytearray(b"".join(words)), dtype=torch.uint8).to(dev)
    idx = torch.randint(0, len(words), (n,), device=dev, generator=g)
    lens = dict_len[idx]
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offs[1:])
    total = int(offs[-1].item())
    assert total < 2 ** 31
    data = torch.empty(total, dtype=torch.uint8, device=dev)
    step = 1 << 22
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        row = torch.repeat_interleave(torch.arange(r0, r1, device=dev), lens[r0:r1])
        within = torch.arange(row.numel(), device=dev) - (offs[row] - offs[r0])
        data[offs[r0]:offs[r1]] = dict_bytes[dict_off[idx[row]] + within]
    return Array(DataType.Utf8, n, data, None, offs.to(torch.int32), 0), total


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
    g.manual_seed(12)
    schema = Schema([Field("k", DataType.Int64, False), Field("s", DataType.Utf8, False)])
    k = torch.randint(0, 10_000, (n,), dtype=torch.int64, device=dev, generator=g) * 1_000_003
    eng = engine(dev)
    key = compile_scalar_expr(None, Column(0), schema, FL)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def aggs(names):
        return [compile_expr(None, AggregateFunction(f, (Column(1),), DataType.UInt64 if f == "COUNT" else DataType.Utf8),
                             schema, FL) for f in names]

    for kind in ("c3", "one", "few", "prefix16"):
        s, nbytes = utf8_column(dev, g, n, dictionary(kind))
        batch = RecordBatch(schema, [Array(DataType.Int64, n, k.view(torch.uint8)), s])
        for grouped in (False, True):
            res = {}
            for tag, names in (("count", ["COUNT"]), ("min_max", ["MIN", "MAX"]), ("count_again", ["COUNT"])):
                cs = aggs(names)
                st = eng.grouped_agg_state([key], cs) if grouped else eng.agg_state(cs)
                ms, all_ms = timed(lambda: st.add(None, batch, FL), iters, before=st.reset)
                res[tag] = ms
                out = st.finish()
                rec = {"column": kind, "grouped_by_10k_keys": grouped, "case": tag, "rows": n, "utf8_bytes": nbytes,
                       "accumulate_ms": round(ms, 3), "min_ms": round(min(all_ms), 3), "max_ms": round(max(all_ms), 3)}
                if tag == "min_max":  # (the values: the probe's answer is checked by eye against the dictionary)
                    vals = [st.value_strings(j) for j in range(2)]
                    rec["first_min"] = vals[0][0].decode("latin-1")
                    rec["first_max"] = vals[1][0].decode("latin-1")
                    rec["groups"] = len(out[0]) if grouped else 1
                    rec["arena_reserved_bytes"] = int(arena_bytes(st.handle))  # the string arena's device allocation
                emit(rec)
            emit({"column": kind, "grouped_by_10k_keys": grouped, "case": "summary",
                  "min_max_over_count": round(res["min_max"] / res["count"], 2),
                  "min_max_minus_count_ms": round(res["min_max"] - res["count"], 3),
                  "count_spread_ms": round(abs(res["count_again"] - res["count"]), 3)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
