"""ORDER BY / LIMIT probe (DESIGN.md §6 "ORDER BY"): a Float64 key with an
Int64 and a Float64 payload, 1e8 rows by default, one device batch.

Times, as the median of --iters HIP-event timings after warm-up:
  * the full sort (dfmi_sort_batches, no limit);
  * LIMIT 100 with the top-k select forced on and forced off;
  * for reference, torch.sort(stable=True) + index_select of the payloads, and
    torch.topk + index_select, on the same device tensors.
Per dfmi call it also prints the device time of each phase (select, key
words, radix passes, gather: DFMI_SORT_PROFILE) with rows/s and the phase's
algorithmic bytes over its time as a fraction of 8 TB/s. The byte model, per
row of the phase's input: key word 8 B read + 8 B written (+ 4 B permutation);
a radix pass over 64-bit words with 32-bit values in 8-bit digits, 8 x (12 B
read + 12 B written) + one 8 B histogram read; select, the 8 B word once per
11-bit pass (6) + count + compaction; gather, 4 B permutation + 8 B read and
8 B written per column.

    python tools/sort_probe.py [--rows N] [--iters K] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

os.environ["DFMI_DIAG"] = "1"
os.environ["DFMI_SORT_PROFILE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema  # noqa: E402
from datafusion_amd.execution.engine import engine  # noqa: E402
from datafusion_amd.logicalplan import DataType  # noqa: E402

PEAK = 8e12  # B/s
PHASES = ["select", "word", "radix", "gather"]


def timed(fn, iters, warmup=2):
    """Median milliseconds of `iters` HIP-event timings of fn()."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def phase_bytes(n, sorted_rows, select, out_rows, ncols=3):
    return {
        "select": n * (8 + 8) + n * 8 * (6 + 2) + sorted_rows * 4 if select else 0,
        "word": sorted_rows * (8 + 8 + 4),
        "radix": sorted_rows * (8 * 24 + 8),
        "gather": out_rows * (4 + 16 * ncols),
    }


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
    key = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    pay_i = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g)
    pay_f = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    schema = Schema([Field("k", DataType.Float64, False), Field("i", DataType.Int64, False),
                     Field("f", DataType.Float64, False)])
    batch = RecordBatch(schema, [Array(DataType.Float64, n, key.view(torch.uint8)),
                                 Array(DataType.Int64, n, pay_i.view(torch.uint8)),
                                 Array(DataType.Float64, n, pay_f.view(torch.uint8))])
    eng = engine(dev)
    L = _abi.lib()
    L.dfmi_internal_sort_phases.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.dfmi_internal_sort_phases.restype = C.c_int32
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def dfmi_case(name, limit, select):
        if select is None:
            os.environ.pop("DFMI_SORT_SELECT", None)
        else:
            os.environ["DFMI_SORT_SELECT"] = select
        phases = {p: [] for p in PHASES}
        out = {}

        def call():
            out["cols"] = eng.sort_batches([batch], [0], [True], limit, _abi.DFMI_FLAG_EXT_SORT)
            ms = (C.c_double * 4)()
            L.dfmi_internal_sort_phases(eng.ctx, ms)
            for p, v in zip(PHASES, ms):
                phases[p].append(v)

        med, _ = timed(call, iters)
        m = out["cols"][0].length
        sel = statistics.median(phases["select"][-iters:]) > 0
        # rows that went through the permutation passes: every row, or the select's candidates (~ the limit)
        sorted_rows = m if sel else n
        by = phase_bytes(n, sorted_rows, sel, m)
        rec = {"case": name, "rows": n, "limit": limit, "select": select, "out_rows": m, "call_ms": round(med, 3),
               "rows_per_s": n / (med * 1e-3)}
        for p in PHASES:
            pm = statistics.median(phases[p][-iters:])
            rec[p + "_ms"] = round(pm, 3)
            if pm > 0:
                rec[p + "_rows_per_s"] = (n if p == "select" else (m if p == "gather" else sorted_rows)) / (pm * 1e-3)
                rec[p + "_frac_of_8TBs"] = round(by[p] / (pm * 1e-3) / PEAK, 4)
        emit(rec)
        return out["cols"]

    full = dfmi_case("full_sort", None, None)
    top_on = dfmi_case("limit100_select_on", 100, "1")
    top_off = dfmi_case("limit100_select_off", 100, "0")

    def torch_sort():
        v, idx = torch.sort(key, stable=True)
        return v, pay_i.index_select(0, idx), pay_f.index_select(0, idx)

    def torch_topk():
        v, idx = torch.topk(key, 100, largest=False, sorted=True)
        return v, pay_i.index_select(0, idx), pay_f.index_select(0, idx)

    med, _ = timed(torch_sort, iters)
    emit({"case": "torch_sort_stable_index_select", "rows": n, "call_ms": round(med, 3), "rows_per_s": n / (med * 1e-3)})
    med, _ = timed(torch_topk, iters)
    emit({"case": "torch_topk100_index_select", "rows": n, "call_ms": round(med, 3), "rows_per_s": n / (med * 1e-3)})

    # the three dfmi results agree with torch's (values bit for bit; distinct keys, so no tie order to compare)
    v, pi, pf = torch_sort()
    as_i64 = lambda a: a.values[: a.length * 8].view(torch.int64)
    ok = bool(torch.equal(as_i64(full[0]), v.view(torch.int64)) and torch.equal(as_i64(full[1]), pi)
              and torch.equal(as_i64(full[2]), pf.view(torch.int64)))
    for top in (top_on, top_off):
        ok = ok and bool(torch.equal(as_i64(top[0]), v[:100].view(torch.int64)) and torch.equal(as_i64(top[1]), pi[:100]))
    emit({"case": "agrees_with_torch", "ok": ok})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
