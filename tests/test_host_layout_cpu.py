"""dfmi_host_batches_output_bytes (no device needed) returns the host-batches
layout's output size: per batch and output a 256-aligned values region, a
validity bitmap in whole 64-bit words and, for Utf8, offsets and the source
column's bytes -- restated here from include/dfmi.h's description."""
import ctypes as C

import numpy as np

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution.engine import column_struct
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator


def align256(x):
    return (x + 255) // 256 * 256


def bitmap_bytes(n):
    return (n + 63) // 64 * 8


def test_output_bytes_is_the_layouts_output_size():
    flags = _abi.DFMI_FLAG_EXT_GATHER_ALL
    s = Schema([Field("f", DataType.Float64, False), Field("b", DataType.Boolean, True),
                Field("s", DataType.Utf8, False), Field("i", DataType.Int8, False)])
    rng = np.random.default_rng(3)
    sizes = [0, 1, 1025]
    batches, want = [], 0
    for n in sizes:
        strings = [b"x" * int(k) for k in rng.integers(0, 5, n)]
        batches.append(RecordBatch(s, [Array.from_numpy(DataType.Float64, rng.random(n)),
                                       Array.from_numpy(DataType.Boolean, rng.random(n) < 0.5, rng.random(n) < 0.9),
                                       Array.from_strings(strings),
                                       Array.from_numpy(DataType.Int8, rng.integers(-5, 5, n).astype(np.int8))]))
        want += align256(n * 8) + align256(bitmap_bytes(n))           # Float64
        want += 2 * align256(bitmap_bytes(n))                         # Boolean: values and validity bitmaps
        want += align256(bitmap_bytes(n)) + align256((n + 1) * 4) + align256(max(sum(map(len, strings)), 1))  # Utf8
        want += align256(n) + align256(bitmap_bytes(n))               # Int8
    want = align256(max(want, 256))
    pred = compile_scalar_expr(None, BinaryExpr(Column(0), Operator.Gt, Literal(Float64(0.25))), s, flags)
    projs = [compile_scalar_expr(None, Column(c), s, flags) for c in range(4)]
    progs = (C.c_void_p * 4)(*[p.handle.value for p in projs])
    keep = []
    barr = (_abi.dfmi_batch * len(batches))()
    for k, b in enumerate(batches):
        carr = (_abi.dfmi_column * 4)(*[column_struct(a) for a in b.columns])
        keep.append(carr)
        barr[k].num_columns, barr[k].num_rows, barr[k].columns = 4, b.num_rows(), carr
    size = C.c_size_t(0)
    err = _abi.dfmi_error()
    rc = _abi.lib().dfmi_host_batches_output_bytes(pred.handle, progs, 4, C.cast(barr, C.c_void_p), len(batches), flags,
                                                   C.byref(size), C.byref(err))
    assert rc == _abi.DFMI_OK, err.message
    assert size.value == want
