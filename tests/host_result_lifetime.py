"""Child process of test_gpu_batches.test_host_results_outlive_their_context
(not collected by pytest): two dfmi_filter_project_host results are read and
freed after their context is destroyed.

Its own process because the library reads whether DFMI_HOST_CHUNK_ROWS is set
once, on the first dfmi_filter_project_host call of a process: the 2,000-row
call in four 512-row chunks has to be that first call, so it runs before the
1024-row one."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema  # noqa: E402
from datafusion_amd.execution.engine import column_struct  # noqa: E402
from datafusion_amd.execution.expression import compile_scalar_expr  # noqa: E402
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator  # noqa: E402


def main():
    L = _abi.lib()
    schema = Schema([Field(c, DataType.Float64, False) for c in "abc"])
    pred = compile_scalar_expr(None, BinaryExpr(
        BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.3))), Operator.And,
        BinaryExpr(Column(1), Operator.Lt, Literal(Float64(0.7)))), schema)
    projs = [compile_scalar_expr(None, e, schema) for e in (
        Column(0), Column(1),
        BinaryExpr(BinaryExpr(Column(0), Operator.Multiply, Column(1)), Operator.Plus, Column(2)))]
    progs = (C.c_void_p * 3)(*[p.handle.value for p in projs])

    ctx = C.c_void_p()
    err = _abi.dfmi_error()
    assert L.dfmi_context_create(0, None, C.byref(ctx), C.byref(err)) == _abi.DFMI_OK, err.message

    rng = np.random.default_rng(5)
    calls = []
    for n, chunk_rows in ((2000, "512"), (1024, None)):
        cols = [rng.random(n) for _ in range(3)]
        batch = RecordBatch(schema, [Array.from_numpy(DataType.Float64, v) for v in cols])
        carr = (_abi.dfmi_column * 3)(*[column_struct(a) for a in batch.columns])
        cb = _abi.dfmi_batch()
        cb.num_columns, cb.num_rows, cb.columns = 3, n, carr
        res = C.c_void_p()
        if chunk_rows:
            os.environ["DFMI_HOST_CHUNK_ROWS"] = chunk_rows
        try:
            rc = L.dfmi_filter_project_host(ctx, pred.handle, progs, 3, C.byref(cb), 0, C.byref(res), C.byref(err))
        finally:
            os.environ.pop("DFMI_HOST_CHUNK_ROWS", None)
        assert rc == _abi.DFMI_OK, err.message
        calls.append((cols, res))

    L.dfmi_context_destroy(ctx)

    for (a, b, c), res in calls:
        keep = (a > 0.3) & (b < 0.7)
        want = [a[keep], b[keep], (a * b + c)[keep]]
        assert L.dfmi_host_result_num_columns(res) == 3
        for i in range(3):
            view = _abi.dfmi_column()
            assert L.dfmi_host_result_column(res, i, C.byref(view)) == _abi.DFMI_OK
            assert view.type == int(DataType.Float64) and view.length == len(want[i]) and view.null_count == 0
            got = np.ctypeslib.as_array(C.cast(view.values, C.POINTER(C.c_uint64)), (view.length,))
            assert np.array_equal(got, want[i].view(np.uint64)), "column %d of the %d-row call" % (i, len(a))
        L.dfmi_host_result_free(res)
    print("results outlived their context")


if __name__ == "__main__":
    main()
