"""compile_scalar_expr / RuntimeExpr (src/execution/expression.rs:29-78, :244-451).

The compiled closure of the reference is replaced by a dfmi_program handle:
compile-time checks, names and types come from libdfmi
(dfmi_compile_scalar_expr), evaluation happens in the fused HIP pass.
"""
from __future__ import annotations

import ctypes as C

from .. import _abi
from ..arrow import Schema
from ..logicalplan import AggregateFunction, Cast, Column, DataType, Expr, Literal
from .error import ExecutionError


class RuntimeExpr:
    """RuntimeExpr::Compiled { name, f, t } — f is a device program."""

    def __init__(self, expr: Expr, handle: int, schema: Schema, flags: int):
        self.expr = expr
        self._handle = C.c_void_p(handle)
        self.flags = flags
        L = _abi.lib()
        self.name = L.dfmi_program_name(self._handle).decode("utf-8", errors="surrogateescape")
        self.t = DataType(L.dfmi_program_type(self._handle))
        self.input_schema = schema

    @property
    def handle(self) -> C.c_void_p:
        return self._handle

    def get_name(self) -> str:
        return self.name

    def get_type(self) -> DataType:
        return self.t

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _abi.lib().dfmi_program_free(h)
            except Exception:
                pass
            self._handle = C.c_void_p(0)


def schema_struct(schema: Schema):
    return _abi.make_schema([(f.name, f.data_type, f.nullable) for f in schema.fields])


class FormatExpr:
    """CAST(e AS Utf8) as the root of a projection (DFMI_FLAG_EXT_CAST with
    DFMI_FLAG_EXT_CAST_UTF8): the fused pass runs the compiled CHILD -- `handle`
    is its program, `child` its RuntimeExpr -- into a fixed-width column, which
    the engine then formats (dfmi_format_utf8_batches). `format` is the mark the
    engine and ProjectRelation look for."""

    format = True

    def __init__(self, expr: Cast, child: RuntimeExpr):
        self.expr = expr
        self.child = child
        self.flags = child.flags
        self.name = repr(expr)  # "CAST(#0 AS Utf8)": expr_debug's text
        self.t = DataType.Utf8
        self.input_schema = child.input_schema

    @property
    def handle(self) -> C.c_void_p:
        return self.child.handle

    def get_name(self) -> str:
        return self.name

    def get_type(self) -> DataType:
        return self.t


_CAST_UTF8 = _abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_CAST_UTF8
_FORMATTED = (DataType.Boolean, DataType.Int8, DataType.Int16, DataType.Int32, DataType.Int64, DataType.UInt8,
              DataType.UInt16, DataType.UInt32, DataType.UInt64, DataType.Float32, DataType.Float64)


def compile_scalar_expr(ctx, expr: Expr, input_schema: Schema, flags: int = None, allow_format: bool = True):
    """expression.rs:244 — raises ExecutionError exactly where the reference's
    compile_scalar_expr returns Err. Under DFMI_FLAG_EXT_CAST_UTF8 a root
    CAST(e AS Utf8) gives a FormatExpr over the compiled child (a Utf8 column
    child: the column itself under the cast's name); allow_format=False -- a
    predicate, an aggregate argument, a GROUP BY key -- leaves such a cast to
    the library, which rejects it as before."""
    if flags is None:
        flags = getattr(ctx, "flags", 0) if ctx is not None else 0
    if (allow_format and (flags & _CAST_UTF8) == _CAST_UTF8 and isinstance(expr, Cast)
            and expr.data_type == DataType.Utf8 and not isinstance(expr.expr, Literal)):
        child = compile_scalar_expr(ctx, expr.expr, input_schema, flags, allow_format=False)
        if child.get_type() == DataType.Utf8 and isinstance(expr.expr, Column):
            child.name = repr(expr)
            return child
        if child.get_type() in _FORMATTED:
            return FormatExpr(expr, child)
        # (anything else: the library's own error below)
    nodes = _abi.PostfixNodes(expr.to_postfix())
    sch, keep = schema_struct(input_schema)
    out = C.c_void_p()
    err = _abi.dfmi_error()
    rc = _abi.lib().dfmi_compile_scalar_expr(nodes.array, nodes.length, C.byref(sch), flags,
                                            C.byref(out), C.byref(err))
    if rc != _abi.DFMI_OK:
        raise ExecutionError.from_status(rc, err.message.decode("utf-8", errors="replace"))
    return RuntimeExpr(expr, out.value, input_schema, flags)


class AggregateExpr:
    """RuntimeExpr::AggregateFunction { name, f, args, t } (expression.rs:51-56):
    a dfmi_aggregate handle over the compiled argument (DFMI_FLAG_EXT_AGGREGATE)."""

    def __init__(self, expr: AggregateFunction, handle: int, arg: RuntimeExpr):
        self.expr = expr
        self.arg = arg
        self._handle = C.c_void_p(handle)
        L = _abi.lib()
        self.name = L.dfmi_aggregate_name(self._handle).decode("utf-8", errors="surrogateescape")
        self.t = DataType(L.dfmi_aggregate_type(self._handle))

    @property
    def handle(self) -> C.c_void_p:
        return self._handle

    def get_name(self) -> str:
        return self.name

    def get_type(self) -> DataType:
        return self.t

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _abi.lib().dfmi_aggregate_free(h)
            except Exception:
                pass
            self._handle = C.c_void_p(0)


def compile_expr(ctx, expr: Expr, input_schema: Schema, flags: int = None):
    """expression.rs:81-116: an AggregateFunction compiles its single argument
    with compile_scalar_expr and maps the name to an AggregateType (anything
    but min/max/count/sum panics); every other expression is
    compile_scalar_expr."""
    if flags is None:
        flags = getattr(ctx, "flags", 0) if ctx is not None else 0
    if not isinstance(expr, AggregateFunction):
        return compile_scalar_expr(ctx, expr, input_schema, flags)
    if len(expr.args) != 1:  # assert_eq!(1, args.len())
        raise ExecutionError("panic", "assertion failed: `(left == right)`\n  left: `1`,\n right: `%d`"
                             % len(expr.args))
    arg = compile_scalar_expr(ctx, expr.args[0], input_schema, flags, allow_format=False)
    out = C.c_void_p()
    err = _abi.dfmi_error()
    rc = _abi.lib().dfmi_compile_aggregate(expr.name.encode("utf-8"), arg.handle, int(expr.return_type), flags,
                                          C.byref(out), C.byref(err))
    if rc != _abi.DFMI_OK:
        raise ExecutionError.from_status(rc, err.message.decode("utf-8", errors="replace"))
    return AggregateExpr(expr, out.value, arg)
