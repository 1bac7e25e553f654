"""Utf8 ordering comparisons (DFMI_FLAG_EXT_UTF8_ORDER) without a GPU: what
the C ABI compiles with and without the two flags, the generated kernels of
every operand form compiled for gfx950 through dfmi_internal_jit_check, the
planner's plan of the prefix-range query, and the comparison core -- the
skeleton's own text -- run on the host under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/native/utf8_order_driver.cpp)."""
import os
import shutil
import subprocess

import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Field, Schema
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator, Utf8
from datafusion_amd.sqlplanner import SqlToRel
from oracle_ffi import oracle_compile
from test_jit_cpu import jit_check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CMP, ORD = _abi.DFMI_FLAG_EXT_UTF8_COMPARE, _abi.DFMI_FLAG_EXT_UTF8_ORDER
BOTH = CMP | ORD
ORDER_OPS = [Operator.Lt, Operator.LtEq, Operator.Gt, Operator.GtEq]
S = Schema([Field("s", DataType.Utf8, True), Field("t", DataType.Utf8, False), Field("v", DataType.Float64, True)])


def lit(b: bytes) -> Literal:
    return Literal(Utf8(b.decode("utf-8", errors="surrogateescape")))


def compiled(e, flags):
    try:
        r = compile_scalar_expr(None, e, S, flags)
        return ("ok", r.get_name(), r.get_type())
    except ExecutionError as x:
        return ("err", x.kind, x.message)


def oracle(e, flags):
    try:
        return ("ok",) + oracle_compile(e, S, flags)
    except ExecutionError as x:
        return ("err", x.kind, x.message)


def test_flag_constant_in_header_binding_and_guide():
    assert ORD == 0x100
    assert "#define DFMI_FLAG_EXT_UTF8_ORDER   0x100u" in open(os.path.join(ROOT, "include", "dfmi.h")).read()
    assert "pub const DFMI_FLAG_EXT_UTF8_ORDER: u32 = 0x100;" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _abi.DFMI_ABI_VERSION == 4 == _abi.lib().dfmi_abi_version()


@pytest.mark.parametrize("op", ORDER_OPS, ids=[o.name for o in ORDER_OPS])
def test_compile_results_with_and_without_the_flags(op):
    forms = [BinaryExpr(Column(0), op, lit(b"w2")), BinaryExpr(lit(b"w2"), op, Column(1)),
             BinaryExpr(Column(0), op, Column(1)), BinaryExpr(lit(b"a"), op, lit(b"b"))]
    for e in forms:
        assert compiled(e, BOTH) == ("ok", repr(e), DataType.Boolean)
        # either flag missing: what the oracle (which knows neither ordering nor the new flag) says today
        assert compiled(e, CMP) == oracle(e, CMP)
        assert compiled(e, ORD) == compiled(e, 0) == oracle(e, 0)
    assert compiled(forms[0], 0) == ("err", "ExecutionError", 'No support for literal type Utf8("w2")')
    # without DFMI_FLAG_EXT_UTF8_ORDER, and for mixed types with it, the node keeps its run-time
    # "comparison_ops" (tests/test_gpu_utf8_order.py runs it): no ordering helper is generated
    for e, fl in ((forms[0], CMP), (BinaryExpr(Column(0), op, Column(2)), BOTH)):
        rc, code, msg, src = jit_check(S, e, [Column(2)], fl)
        assert rc > 0, msg
        body = src[src.rindex('extern "C" __global__'):]
        assert "utf8_cmp_" not in body and "utf8_ord<" not in body


def range_pred(lo=b"w2", hi=b"w3"):
    return BinaryExpr(BinaryExpr(Column(0), Operator.GtEq, lit(lo)), Operator.And,
                      BinaryExpr(Column(0), Operator.Lt, lit(hi)))


SHAPES = {
    "utf8_only_predicate": (range_pred(), [Column(0), Column(2)]),
    "mixed_predicate": (BinaryExpr(BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5))), Operator.And,
                                   BinaryExpr(Column(0), Operator.GtEq, lit(b"abc"))), [Column(0), Column(2)]),
    "literal_on_the_left": (BinaryExpr(lit(b"m"), Operator.LtEq, Column(0)), [Column(0)]),
    "column_column": (BinaryExpr(Column(0), Operator.Gt, Column(1)), [Column(1), Column(2)]),
    "projection": (None, [BinaryExpr(Column(0), Operator.Lt, lit(b"abcd")), Column(0),
                          BinaryExpr(Column(1), Operator.GtEq, Column(0)), BinaryExpr(lit(b"a"), Operator.Lt, lit(b"b"))]),
    "projection_after_selection": (BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5))),
                                   [BinaryExpr(Column(0), Operator.Lt, lit(b"abcd")), Column(0)]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernels_compile_for_gfx950(shape):
    pred, projs = SHAPES[shape]
    rc, code, msg, src = jit_check(S, pred, projs, BOTH, compile_=True)
    assert rc > 0, msg
    assert "utf8_cmp_" in src.split("// ---- utf8 order core: end")[-1] or shape == "utf8_only_predicate"
    if shape in ("utf8_only_predicate", "mixed_predicate"):  # the tile pre-pass, once per comparison
        body = src[src.rindex('extern "C" __global__'):]
        # (the range's two bounds share one fetch of the heads)
        assert body.count("dfmi::utf8_cmp_lits_tile<BLOCK, K, 4, 2>") == (shape == "utf8_only_predicate")
        assert body.count("dfmi::utf8_cmp_lit_tile<BLOCK, K, 4>") == (shape == "mixed_predicate")


@pytest.mark.parametrize("form,bit", [("one_tile", 0x20000000), ("coalesced_batches", 0x40000000)])
def test_other_kernel_forms_compile(form, bit):
    """The hook's internal flag bits: the one-tile kernel a Utf8-only predicate switches to once it
    selected most of a large batch (exec_plan.cpp high_sel), and the coalesced-batches form."""
    default = jit_check(S, range_pred(), [Column(0), Column(2)], BOTH)[3]
    rc, code, msg, src = jit_check(S, range_pred(), [Column(0), Column(2)], BOTH | bit, compile_=True)
    assert rc > 0, msg
    assert src != default and "utf8_cmp_lits_tile<BLOCK, K, " in src[src.rindex('extern "C" __global__'):]
    assert "constexpr int M = 8;" in default and (form != "one_tile" or "constexpr int M = 8;" not in src)


@pytest.mark.parametrize("h,pre", [(8, 1), (8, 0), (4, 0)])
def test_diagnostic_variants_compile(h, pre, monkeypatch):
    """Head width 8 and the per-row form inside the predicate loop (DFMI_DIAG knobs)."""
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_UTF8_ORD_H", str(h))
    monkeypatch.setenv("DFMI_UTF8_ORD_PRE", str(pre))
    rc, code, msg, src = jit_check(S, range_pred(), [Column(0), Column(2)], BOTH, compile_=True)
    assert rc > 0, msg
    body = src[src.rindex('extern "C" __global__'):]
    assert ("utf8_cmp_lits_tile<BLOCK, K, %d, 2>" % h in body) == bool(pre)
    assert ("utf8_cmp_lit<5, %d>" % h in body) == (not pre)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 8, 9, 200])
def test_literal_lengths_compile_and_are_kernel_arguments(n):
    a, b = bytes(97 + i % 26 for i in range(n)), bytes(65 + i % 26 for i in range(n))
    pa = BinaryExpr(Column(0), Operator.Lt, lit(a))
    rc, code, msg, src = jit_check(S, pa, [Column(0), Column(2)], BOTH, compile_=True)
    assert rc > 0, msg
    rc2, _, msg2, src2 = jit_check(S, BinaryExpr(Column(0), Operator.Lt, lit(b)), [Column(0), Column(2)], BOTH)
    assert rc2 > 0, msg2
    assert src2 == src  # another literal of the same length: the same kernel


def test_literal_pool_limits_stand():
    over = BinaryExpr(BinaryExpr(Column(0), Operator.Lt, lit(b"x" * 200)), Operator.And,
                      BinaryExpr(Column(0), Operator.Gt, lit(b"y" * 57)))
    rc, code, msg, _ = jit_check(S, over, [Column(2)], BOTH)
    assert rc < 0 and code == _abi.DFMI_ERR_NOT_IMPLEMENTED and "string literals too long" in msg


def test_planner_plans_the_prefix_range():
    ctx = ExecutionContext(flags=BOTH)
    ctx.register_datasource("t", MemoryDataSource(Schema([Field("s", DataType.Utf8, True),
                                                          Field("v", DataType.Float64, True)]), []))
    plan = SqlToRel(ctx).sql_to_rel("SELECT s, v FROM t WHERE s >= 'w2' AND s < 'w3'")
    assert repr(plan.input.expr) == '#0 GtEq Utf8("w2") And #0 Lt Utf8("w3")'
    assert [repr(e) for e in plan.expr] == ["#0", "#1"]
    assert type(plan).__name__ == "Projection" and type(plan.input).__name__ == "Selection"


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_comparison_core_and_front_end_under_asan_ubsan(tmp_path):
    skel = open(os.path.join(ROOT, "datafusion_amd", "csrc", "jit_skeleton.hip")).read()
    begin, end = "// ---- utf8 order core: begin", "// ---- utf8 order core: end"
    assert skel.count(begin) == 1 and skel.count(end) == 1
    core = skel[skel.index(begin):skel.index(end)]
    assert "Args" not in core.replace("no Args", "") and "__builtin_amdgcn" not in core.split("#endif", 1)[1]
    (tmp_path / "utf8_order_core.inc").write_text(core)
    out = str(tmp_path / "utf8_order_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", str(tmp_path), "-o", out,
           os.path.join(HERE, "native", "utf8_order_driver.cpp"),
           os.path.join(ROOT, "datafusion_amd", "csrc", "compile.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "utf8 order driver: clean" in r.stdout and "1000000 random pairs" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
