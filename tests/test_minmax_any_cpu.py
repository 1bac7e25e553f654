"""MIN / MAX over a Boolean or Utf8 argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY)
without a GPU: the front end's compile matrix, the header and the binding,
the aggregate kernels with a Boolean extreme generated and compiled for
gfx950 (a Utf8 extreme shares COUNT's source), Boolean partials merged by
hand through dfmi_agg_merge_partials, the refusal of a Utf8 extreme's
partial, and the host code under the sanitizers
(tests/native/minmax_any_driver.cpp).

Build-defined: the reference plans MIN / MAX of any type (sqlplanner.rs:296,
return type = argument type) and executes no Aggregate; parity is pinned only
by the Boolean and Utf8 cells of its aggregate fixtures
(tests/test_gpu_minmax_any.py)."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Field, Schema
from datafusion_amd.execution.engine import merge_agg_partials
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_expr
from datafusion_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Float64, Literal, Operator
from test_aggregate_cpu import _agg_jit, _grouped_jit, agg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

AGG = _abi.DFMI_FLAG_EXT_AGGREGATE
ANY = AGG | _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY
LIMBS = 68
AGGF_VALUE = 16

S = Schema([Field("c0", DataType.Boolean, True), Field("c11", DataType.Utf8, True), Field("x", DataType.Float64, True),
            Field("k", DataType.Int16, True), Field("kb", DataType.Boolean, True)])


def _error(name, col, flags, ret=None):
    e = agg(name, Column(col), S) if ret is None else AggregateFunction(name, (Column(col),), ret)
    with pytest.raises(ExecutionError) as ei:
        compile_expr(None, e, S, flags)
    return ei.value.kind, ei.value.message


# ------------------------------------------------------------------ front end
def test_compile_matrix():
    # without the new flag: today's code and text, whatever else is set
    for flags in (AGG, AGG | _abi.DFMI_FLAG_EXT_AGG_AVG | _abi.DFMI_FLAG_EXT_UTF8_ORDER | _abi.DFMI_FLAG_EXT_UTF8_COMPARE):
        assert _error("MIN", 0, flags) == ("NotImplemented", "aggregate over Boolean")
        assert _error("MAX", 1, flags) == ("NotImplemented", "aggregate over Utf8")
    # the new flag alone is not the aggregate extension
    assert _error("MIN", 0, _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY) == ("panic", "not yet implemented")
    assert _error("MAX", 1, _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY) == ("panic", "not yet implemented")
    # with both: a Boolean / Utf8 extreme compiles, its type the argument's
    for name in ("MIN", "max", "Min", "mAX"):
        a = compile_expr(None, agg(name, Column(0), S), S, ANY)
        assert a.get_name() == name and a.get_type() == DataType.Boolean
        a = compile_expr(None, agg(name, Column(1), S), S, ANY)
        assert a.get_name() == name and a.get_type() == DataType.Utf8
    e = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5)))
    assert compile_expr(None, agg("MAX", e, S), S, ANY).get_type() == DataType.Boolean
    # SUM and AVG over Boolean keep their errors
    both = ANY | _abi.DFMI_FLAG_EXT_AGG_AVG
    for col, tname in ((0, "Boolean"), (1, "Utf8")):
        for name in ("SUM", "AVG"):
            assert _error(name, col, both) == ("NotImplemented", "aggregate over " + tname)
    # a wrong return type
    for t in (DataType.UInt8, DataType.UInt64, DataType.Utf8):
        assert _error("MIN", 0, ANY, t) == ("InvalidArgument", "aggregate return type does not match the planner's")
    for t in (DataType.Boolean, DataType.UInt64):
        assert _error("MAX", 1, ANY, t) == ("InvalidArgument", "aggregate return type does not match the planner's")
    # COUNT and the numeric aggregates are untouched by the flag
    assert compile_expr(None, agg("COUNT", Column(0), S), S, ANY).get_type() == DataType.UInt64
    assert compile_expr(None, agg("MIN", Column(3), S), S, ANY).get_type() == DataType.Int16


def test_header_and_binding_declare_the_flag():
    h = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    assert re.search(r"#define\s+DFMI_FLAG_EXT_AGG_MINMAX_ANY\s+0x200u", h)
    assert re.search(r"#define DFMI_ABI_VERSION 4\b", h)
    assert _abi.DFMI_FLAG_EXT_AGG_MINMAX_ANY == 0x200
    assert _abi.DFMI_ABI_VERSION == 4 and _abi.lib().dfmi_abi_version() == 4


def test_planner_builds_boolean_extremes():
    from datafusion_amd.execution import ExecutionContext, MemoryDataSource
    from datafusion_amd.execution.context import Aggregate
    from datafusion_amd.sqlplanner import SqlToRel
    ctx = ExecutionContext(flags=ANY)
    ctx.register_datasource("t", MemoryDataSource(S, []))
    p = SqlToRel(ctx).sql_to_rel("SELECT k, MIN(c0), MAX(c0), MIN(c11) FROM t GROUP BY k")
    assert isinstance(p, Aggregate)
    assert [e.return_type for e in p.aggr_expr] == [DataType.Boolean, DataType.Boolean, DataType.Utf8]
    for e in p.aggr_expr:
        assert compile_expr(ctx, e, S).get_type() == e.return_type


# -------------------------------------------------------------------- kernels
def test_kernels_with_a_boolean_extreme_compile():
    """The ungrouped and the window kernels (Int16 and Boolean key), in the
    one-tile and the coalesced form, with and without a predicate: a Boolean
    extreme is fed to agg_key as an unsigned byte 0 / 1."""
    fl = ANY | _abi.DFMI_FLAG_EXT_GATHER_ALL
    e = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5)))
    aggs = [agg("MIN", Column(0), S), agg("max", Column(0), S), agg("SUM", Column(2), S), agg("COUNT", Column(0), S),
            agg("MIN", e, S), agg("MAX", Column(3), S)]
    pred = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.7)))
    for p in (None, pred):
        for form in (0, 0x40000000):  # one tile per batch / coalesced batches
            rc, code, msg, src = _agg_jit(S, p, aggs, fl | form)
            assert rc > 0, msg
            assert src.count("dfmi::agg_key((unsigned char)((") == 3
            for key in (Column(3), Column(4)):
                rc, code, msg, gsrc = _grouped_jit(S, p, key, aggs, fl | form)
                assert rc > 0, msg
                assert gsrc.count("dfmi::agg_key((unsigned char)((") == 3
    # a Utf8 extreme is a COUNT inside the kernels: the source (and the code object) of COUNT in its place
    with_s = [agg("MIN", Column(1), S), agg("SUM", Column(2), S), agg("MAX", Column(1), S)]
    as_count = [agg("COUNT", Column(1), S), agg("SUM", Column(2), S), agg("COUNT", Column(1), S)]
    for p in (None, pred):
        rc, code, msg, src = _agg_jit(S, p, with_s, fl)
        assert rc > 0, msg
        assert src == _agg_jit(S, p, as_count, fl, compile_=False)[3]
    # the numeric kernels' text does not depend on the flag
    num = [agg("MIN", Column(3), S), agg("SUM", Column(2), S)]
    assert _agg_jit(S, pred, num, fl, compile_=False)[3] == \
        _agg_jit(S, pred, num, AGG | _abi.DFMI_FLAG_EXT_GATHER_ALL, compile_=False)[3]


# ------------------------------------------------------------------- partials
def partial(count: int, key: int = 0, has_value: bool = False) -> bytes:
    """aggh::Partial: count, flags, key, isum, then the 68 digits."""
    return struct.pack("<4Q", count, AGGF_VALUE if has_value else 0, key, 0) + struct.pack("<%dq" % LIMBS, *([0] * LIMBS))


def test_boolean_partials_merge_as_integer_extremes():
    mn = compile_expr(None, agg("MIN", Column(0), S), S, ANY)
    mx = compile_expr(None, agg("MAX", Column(0), S), S, ANY)
    empty_min, empty_max = partial(0, 2 ** 64 - 1), partial(0, 0)  # (a state's zero state: MIN keys all ones)
    cases = [
        ([(3, 1), (2, 0)], 5, 0, 1),
        ([(3, 1), (4, 1)], 7, 1, 1),
        ([(1, 0), (9, 0), (2, 0)], 12, 0, 0),
        ([(5, 0)], 5, 0, 0),
    ]
    for parts, count, want_min, want_max in cases:
        for a, want, empty in ((mn, want_min, empty_min), (mx, want_max, empty_max)):
            blobs = [partial(c, k, True) for c, k in parts] + [empty]
            for order in (blobs, blobs[::-1]):
                (v,) = merge_agg_partials([a], order)
                assert (DataType(v.type), v.is_null, v.count, v.bits) == (DataType.Boolean, 0, count, want)
    for a, empty in ((mn, empty_min), (mx, empty_max)):
        (v,) = merge_agg_partials([a], [empty, empty])
        assert (DataType(v.type), v.is_null, v.count, v.bits) == (DataType.Boolean, 1, 0, 0)


def test_utf8_extreme_partials_are_refused():
    mx = compile_expr(None, agg("MAX", Column(1), S), S, ANY)
    cnt = compile_expr(None, agg("COUNT", Column(1), S), S, ANY)
    with pytest.raises(ExecutionError) as ei:
        merge_agg_partials([cnt, mx], [partial(1) + partial(1)])
    assert (ei.value.kind, ei.value.message) == ("NotImplemented", "partial state of a Utf8 MIN / MAX aggregate")


# ----------------------------------------------------------------- sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_code_under_asan_ubsan(tmp_path):
    out = str(tmp_path / "minmax_any_driver")
    csrc = os.path.join(ROOT, "datafusion_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", out,
           os.path.join(HERE, "native", "minmax_any_driver.cpp"), os.path.join(csrc, "agg_host.cpp"),
           os.path.join(csrc, "compile.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "minmax any driver: clean" in r.stdout
