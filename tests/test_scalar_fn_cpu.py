"""Scalar function extension (DFMI_FLAG_EXT_SCALAR_FUNCTIONS), the parts that
need no GPU: unchanged behaviour without the flag, the registry entry point,
the compile front end's names, types and errors, planning through
function_meta, the wire format, and the ABI surface."""
import ctypes as C
import os
import re

import pytest

from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Field, Schema
from datafusion_amd.execution import ExecutionContext, ExecutionError, MemoryDataSource
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.logicalplan import (BinaryExpr, Cast, Column, DataType, Float64, Int64, Literal, Operator,
                                        PlanError, ScalarFunction)
from datafusion_amd.sqlplanner import SqlToRel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = _abi.DFMI_FLAG_EXT_SCALAR_FUNCTIONS

S = Schema([Field("c0", DataType.Float64, True), Field("c_int", DataType.Int64, True),
            Field("c_f64", DataType.Float64, False), Field("c_f32", DataType.Float32, True),
            Field("s", DataType.Utf8, True)])
NAMES = {"sqrt": 1, "abs": 1, "floor": 1, "ceil": 1, "round": 1, "trunc": 1, "mod": 2}


def context(flags):
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(S, []))
    return ctx


def fn(name, *args, rt=DataType.Float64):
    return ScalarFunction(name, tuple(args), rt)


def compile_err(e, flags):
    with pytest.raises(ExecutionError) as x:
        compile_scalar_expr(None, e, S, flags)
    return x.value.kind, x.value.message


# ------------------------------------------------------------ without the flag
@pytest.mark.parametrize("flags", [0, _abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_AGGREGATE])
def test_without_the_flag_the_compile_error_is_unchanged(flags):
    assert compile_err(fn("sqrt", Column(0)), flags) == ("ExecutionError", "expression sqrt(#0)")
    assert compile_err(fn("mod", Column(0), Literal(Float64(3.0))), flags) == \
        ("ExecutionError", "expression mod(#0, Float64(3.0))")
    assert compile_err(fn("nosuch", Column(0)), flags) == ("ExecutionError", "expression nosuch(#0)")


@pytest.mark.parametrize("flags", [0, _abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_AGGREGATE])
def test_without_the_flag_function_meta_still_panics(flags):
    ctx = context(flags)
    for call in (lambda: ctx.function_meta("sqrt"), lambda: ctx.sql("SELECT sqrt(c0) FROM t")):
        with pytest.raises(ExecutionError) as e:
            call()
        assert (e.value.kind, e.value.message) == ("panic", "not yet implemented")


# --------------------------------------------------------------- the registry
def meta(name: bytes, max_args=4):
    L = _abi.lib()
    args = (C.c_int32 * 4)(-1, -1, -1, -1)
    n, rt = C.c_int32(-1), C.c_int32(-1)
    rc = L.dfmi_scalar_function_meta(name, len(name), args, max_args, C.byref(n), C.byref(rt))
    return rc, list(args), n.value, rt.value


@pytest.mark.parametrize("name", sorted(NAMES))
def test_function_meta_entry_point_knows_the_built_ins(name):
    f64 = int(DataType.Float64)
    rc, args, n, rt = meta(name.encode())
    assert rc == 0 and n == NAMES[name] and rt == f64
    assert args == [f64] * n + [-1] * (4 - n)
    ctx = context(FN)
    assert ctx.function_meta(name) == ([DataType.Float64] * n, DataType.Float64)


def test_function_meta_entry_point_rejects_unknown_names():
    for name in (b"exp", b"SQRT", b"sqr", b"sqrtx", b"", b"pow"):
        rc, args, n, rt = meta(name)
        assert rc != 0 and (args, n, rt) == ([-1] * 4, -1, -1), name
    assert context(FN).function_meta("exp") is None
    # a short caller array is not overrun; NULL outputs are skipped
    rc, args, n, rt = meta(b"mod", max_args=1)
    assert rc == 0 and n == 2 and args == [int(DataType.Float64), -1, -1, -1]
    assert _abi.lib().dfmi_scalar_function_meta(b"mod", 3, None, 0, None, None) == 0


# ----------------------------------------------------------- compile front end
def test_program_name_and_type():
    r = compile_scalar_expr(None, fn("sqrt", Cast(Column(1), DataType.Float64)), S, FN | _abi.DFMI_FLAG_EXT_CAST)
    assert (r.get_name(), r.get_type()) == ("sqrt(CAST(#1 AS Float64))", DataType.Float64)
    r = compile_scalar_expr(None, fn("mod", Column(0), Cast(Literal(Int64(3)), DataType.Float64)), S, FN)
    assert (r.get_name(), r.get_type()) == ("mod(#0, CAST(Int64(3) AS Float64))", DataType.Float64)
    # nested, inside operators, and as a predicate's operand
    e = BinaryExpr(fn("floor", BinaryExpr(fn("abs", Column(0)), Operator.Multiply, Column(2))), Operator.Lt,
                   Literal(Float64(0.5)))
    r = compile_scalar_expr(None, e, S, FN)
    assert (r.get_name(), r.get_type()) == ("floor(abs(#0) Multiply #2) Lt Float64(0.5)", DataType.Boolean)


def test_the_three_error_texts():
    assert compile_err(fn("exp", Column(0)), FN) == ("ExecutionError", "Invalid function 'exp'")
    assert compile_err(fn("SQRT", Column(0)), FN) == ("ExecutionError", "Invalid function 'SQRT'")
    assert compile_err(fn("sqrt", Column(0), Column(2)), FN) == \
        ("ExecutionError", "Function 'sqrt' expects 1 arguments, got 2")
    assert compile_err(fn("mod", Column(0)), FN) == ("ExecutionError", "Function 'mod' expects 2 arguments, got 1")
    assert compile_err(fn("sqrt"), FN) == ("ExecutionError", "Function 'sqrt' expects 1 arguments, got 0")
    assert compile_err(fn("sqrt", Column(1)), FN) == \
        ("ExecutionError", "Function 'sqrt' is not supported for (Int64) -> Float64")
    assert compile_err(fn("abs", Column(4)), FN | _abi.DFMI_FLAG_EXT_UTF8_COMPARE) == \
        ("ExecutionError", "Function 'abs' is not supported for (Utf8) -> Float64")
    assert compile_err(fn("sqrt", Column(0), rt=DataType.Int64), FN) == \
        ("ExecutionError", "Function 'sqrt' is not supported for (Float64) -> Int64")
    # an argument's own compile error comes first (it is compiled first)
    assert compile_err(fn("sqrt", Cast(Column(1), DataType.Float64)), FN) == ("ExecutionError", "column reference")


def test_float32_is_accepted_and_mixed_widths_are_rejected():
    for name, n in NAMES.items():
        r = compile_scalar_expr(None, fn(name, *[Column(3)] * n, rt=DataType.Float32), S, FN)
        assert (r.get_name(), r.get_type()) == ("%s(%s)" % (name, ", ".join(["#3"] * n)), DataType.Float32)
    assert compile_err(fn("sqrt", Column(3)), FN) == \
        ("ExecutionError", "Function 'sqrt' is not supported for (Float32) -> Float64")
    assert compile_err(fn("sqrt", Column(0), rt=DataType.Float32), FN) == \
        ("ExecutionError", "Function 'sqrt' is not supported for (Float64) -> Float32")
    assert compile_err(fn("mod", Column(3), Column(0), rt=DataType.Float64), FN) == \
        ("ExecutionError", "Function 'mod' is not supported for (Float32, Float64) -> Float64")
    assert compile_err(fn("mod", Column(0), Column(3), rt=DataType.Float32), FN) == \
        ("ExecutionError", "Function 'mod' is not supported for (Float64, Float32) -> Float32")


# ------------------------------------------------------- generated kernels
def test_function_kernels_compile_for_gfx950():
    """The kernels the device path would launch, generated and compiled with
    hipRTC (no device): functions in a predicate and in projections after a
    Selection, and a projection-only Float32 form of every function."""
    from test_jit_cpu import jit_check
    f3 = Schema([Field(c, DataType.Float64, c != "b") for c in "abc"])
    pred = BinaryExpr(BinaryExpr(fn("sqrt", Column(0)), Operator.Lt, Literal(Float64(0.5))), Operator.And,
                      BinaryExpr(fn("floor", BinaryExpr(Column(1), Operator.Multiply, Literal(Float64(10.0)))),
                                 Operator.GtEq, Literal(Float64(3.0))))
    projs = [fn("round", Column(2)), fn("mod", Column(0), Literal(Float64(3.0))), Column(1)]
    rc, code, msg, src = jit_check(f3, pred, projs, FN, compile_=True)
    assert rc > 0, msg
    for helper in ("dfmi::fn_sqrt<double>(", "dfmi::fn_floor<double>(", "dfmi::fn_round<double>(",
                   "dfmi::fn_mod<double>("):
        assert helper in src, helper
    g = Schema([Field("x", DataType.Float32, True), Field("y", DataType.Float32, False)])
    projs = [fn(nm, *[Column(0), Column(1)][:n], rt=DataType.Float32) for nm, n in sorted(NAMES.items())]
    rc, code, msg, src = jit_check(g, None, projs, FN, compile_=True)
    assert rc > 0, msg
    for nm in NAMES:
        assert "dfmi::fn_%s<float>(" % nm in src, nm


# ------------------------------------------------------------------- planning
SQL = "SELECT sqrt(c_int), mod(c_f64, 3) FROM t"
DEBUG = ("Projection: sqrt(CAST(#1 AS Float64)), mod(#2, CAST(Int64(3) AS Float64))\n"
         "  TableScan: t projection=None")


def test_planning_casts_each_argument_to_the_declared_type():
    ctx = context(FN | _abi.DFMI_FLAG_EXT_CAST)
    plan = SqlToRel(ctx).sql_to_rel(SQL)
    assert repr(plan) == DEBUG
    assert [(f.name, f.data_type) for f in serde.plan_schema(plan).fields] == \
        [("sqrt", DataType.Float64), ("mod", DataType.Float64)]
    rel = ctx.execute(plan)  # compiles both projections; nothing runs
    assert [(f.name, f.data_type, f.nullable) for f in rel.schema().fields] == \
        [("sqrt", DataType.Float64, True), ("mod", DataType.Float64, True)]
    with pytest.raises(PlanError) as e:
        SqlToRel(ctx).sql_to_rel("SELECT exp(c0) FROM t")
    assert str(e.value) == "Invalid function 'exp'"


def test_serde_round_trip_of_the_plan():
    plan = SqlToRel(context(FN | _abi.DFMI_FLAG_EXT_CAST)).sql_to_rel(SQL)
    wire = serde.to_json(plan)
    assert '"ScalarFunction"' in wire and '"name":"sqrt"' in wire.replace(" ", "")
    back = serde.from_json(wire)
    assert repr(back) == DEBUG
    assert serde.to_json(back) == wire
    assert back.expr == plan.expr


# ------------------------------------------------------------------------ ABI
def test_flag_and_entry_point_are_declared_and_the_version_stays_4():
    hdr = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    m = re.search(r"#define\s+DFMI_FLAG_EXT_SCALAR_FUNCTIONS\s+(0x[0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == _abi.DFMI_FLAG_EXT_SCALAR_FUNCTIONS == 0x40
    assert re.search(r"int32_t\s+dfmi_scalar_function_meta\s*\(", hdr)
    assert re.search(r"#define DFMI_ABI_VERSION 4\b", hdr)
    assert "dfmi_scalar_function_meta" in _abi.EXPORTED
    assert _abi.DFMI_ABI_VERSION == 4 and _abi.lib().dfmi_abi_version() == 4
