#!/usr/bin/env python3
"""Utf8 ordering diagnostics: one 1.25e8-row C3 batch (bench.py's generator,
the 1,000-word `w<i>...` dictionary), `SELECT s, v WHERE s < L` with L chosen
from the sorted dictionary for about 1 %, 50 % and 99 % selectivity, and the
50 % query once more with an empty projection list, each timed under several
environment variants in one process (the query compiler reads its diagnostic
knobs per call and keys its cache on them). Warm-up rule of tools/c3_probe.py:
untimed calls for >= 0.5 s per variant and query (>= 20 s for the first).

Formula bytes per batch: 4 B/row of offsets, every 128-byte line of the
string bytes once (the predicate reads every row's head: all of them), and
the output traffic -- per selected row 8.125 B of v read, 12 B of offset + v
written, and the selected strings' bytes written. The fraction is of 8 TB/s.

usage: tools/utf8_order_probe.py [VAR=VAL[,VAR=VAL...] ...]   (each arg one variant; '-' = defaults)
  DFMI_UTF8_ORD_H=4|8     head bytes compared as one integer (default 4)
  DFMI_UTF8_ORD_PRE=0|1   0: the per-row helper inside the predicate loop
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Field, Schema  # noqa: E402
from datafusion_amd.execution.engine import column_struct, engine  # noqa: E402
from datafusion_amd.execution.expression import compile_scalar_expr  # noqa: E402
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Literal, Operator, Utf8  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = engine(dev)
    words = bench._utf8_dictionary(bench.SEED)
    dict_bytes = torch.tensor(np.frombuffer(b"".join(words), dtype=np.uint8), device=dev)
    dict_len = torch.tensor([len(w) for w in words], dtype=torch.int64, device=dev)
    dict_off = torch.cumsum(dict_len, 0) - dict_len
    g = torch.Generator(device=dev)
    g.manual_seed(bench.SEED + 1000)
    nb = bench.C3_ROWS // bench.C3_BATCHES
    b, nbytes = bench._c3_batch(dev, g, nb, dict_bytes, dict_off, dict_len)
    torch.cuda.empty_cache()
    schema = Schema([Field("s", DataType.Utf8, False), Field("v", DataType.Float64, True)])
    out_s_off = torch.zeros(nb + 16, dtype=torch.int32, device=dev)
    out_s_data = torch.empty(b[0].values.numel(), dtype=torch.uint8, device=dev)
    out_v = torch.empty(nb, dtype=torch.float64, device=dev)
    L = _abi.lib()
    F = _abi.DFMI_FLAG_EXT_UTF8_COMPARE | _abi.DFMI_FLAG_EXT_UTF8_ORDER
    srt = sorted(words)
    bound = {"1%": srt[len(srt) // 100], "50%": srt[len(srt) // 2], "99%": srt[len(srt) * 99 // 100]}
    queries = [(k, w, 2) for k, w in bound.items()] + [("50% no projections", bound["50%"], 0)]
    variants = sys.argv[1:] or ["-"]
    ref = {}
    warmed = False
    for var in variants:
        env = {}
        if var != "-":
            env["DFMI_DIAG"] = "1"  # the library reads its diagnostic knobs only then
            for kv in var.split(","):
                k, v = kv.split("=", 1)
                env[k] = v
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        line = [var]
        for qn, bound_word, nproj in queries:
            pred = compile_scalar_expr(None, BinaryExpr(Column(0), Operator.Lt, Literal(Utf8(bound_word.decode()))),
                                       schema, F)
            projs = [compile_scalar_expr(None, Column(j), schema, F) for j in range(nproj)]
            progs = (C.c_void_p * 2)(*[p.handle.value for p in projs])
            carr = (_abi.dfmi_column * 2)(column_struct(b[0]), column_struct(b[1]))
            cb = _abi.dfmi_batch(2, 0, nb, carr)
            outs = (_abi.dfmi_out_column * 2)()
            outs[0].offsets = out_s_off.data_ptr()
            outs[0].data = out_s_data.data_ptr()
            outs[0].data_capacity = out_s_data.numel()
            outs[1].values = out_v.data_ptr()
            err = _abi.dfmi_error()
            ks, names = [], set()
            t_end = None
            it = 0
            while True:
                rc = L.dfmi_filter_project(eng.ctx, pred.handle, progs, nproj, C.byref(cb), outs, F, C.byref(err))
                if rc != 0:
                    break
                if it == 0:
                    torch.cuda.synchronize()
                    t_end = time.perf_counter() + (0.5 if warmed else 20.0)
                elif time.perf_counter() >= t_end:
                    ks.append(eng.last_timing()[1])
                    names.add(L.dfmi_last_kernel_name(eng.ctx))
                    if len(ks) >= 12:
                        break
                it += 1
            warmed = True
            if rc != 0:
                line.append("%s error: %s" % (qn, err.message.decode()))
                continue
            sel, sb = outs[0].length, outs[0].data_length
            ck = (int(out_s_off[: sel + 1].to(torch.int64).sum().item()),
                  int(out_s_data[:sb].to(torch.int64).sum().item()),
                  int(out_v[:sel].view(torch.int64).sum().item()))
            ref.setdefault(qn, ck)
            alg = nb * 4.0 + nbytes + sel * (8.125 + 12.0) + sb
            ms = float(np.median(ks))
            line.append("%s %.4f ms (min %.4f max %.4f) frac %.3f sel %d %s kernels %d" % (
                qn, ms, min(ks), max(ks), alg / (ms * 1e-3) / 8e12, sel, "same" if ck == ref[qn] else "DIFF", len(names)))
        print(" | ".join(line), flush=True)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


if __name__ == "__main__":
    main()
