#!/usr/bin/env python3
"""Digest of the query compiler's generated source over a fixed corpus of
query shapes: one line `<sha256 of the source> <shape name>` per shape, in a
fixed order (a shape the library refuses: `refused <code> <shape name>`).
No device is needed: the sources come from the library's internal hooks with
compile=0. A kernel's name, the on-disk code objects and the module cache are
all keyed by this text, so two builds with equal digests launch the same
kernels; after a change to the generator or the skeleton, a diff of two runs
names exactly the shapes whose kernels changed.
usage: tools/jit_digest.py > digest.txt"""
import hashlib
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import compose_cases as cc  # noqa: E402
import test_agg_batches_cpu as tb  # noqa: E402
import test_cast_any_cpu as ta  # noqa: E402
import test_jit_cpu as tj  # noqa: E402
import test_minmax_any_cpu as tm  # noqa: E402
import test_modulus_cpu as tmod  # noqa: E402
import test_scalar_fn_cpu as tf  # noqa: E402
import test_utf8_order_cpu as tu  # noqa: E402
from datafusion_amd import _abi  # noqa: E402
from datafusion_amd.arrow import Field, Schema  # noqa: E402
from datafusion_amd.execution.error import ExecutionError  # noqa: E402
from datafusion_amd.execution.expression import compile_scalar_expr  # noqa: E402
from datafusion_amd.logicalplan import (AggregateFunction, BinaryExpr, Cast, Column, DataType, Float64, Int64,  # noqa: E402
                                        IsNotNull, IsNull, Literal, Operator, ScalarValue, Utf8)
from test_aggregate_cpu import AGG, _agg_jit, _grouped_jit, agg  # noqa: E402
from test_jit_cpu import F3, NARROW, S, c2_query, jit_check  # noqa: E402

BATCHED, HIGH_SEL = 0x40000000, 0x20000000
GA = _abi.DFMI_FLAG_EXT_GATHER_ALL
C3 = Schema([Field("s", DataType.Utf8, False), Field("v", DataType.Float64, True)])
COUNT = 0


def line(name, result):
    global COUNT
    rc, code, _msg, src = result
    COUNT += 1
    if rc < 0:
        print("refused %d %s" % (code, name))
    else:
        assert rc < (1 << 20), "source longer than the helpers' buffer"
        print("%s %s" % (hashlib.sha256(src.encode()).hexdigest(), name))


class env:
    """Diagnostic knobs for the calls inside (the library reads them per call)."""

    def __init__(self, **kv):
        self.kv = dict(kv, DFMI_DIAG="1") if kv else {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def filt(name, schema, pred, projs, flags=0, forms=(0, BATCHED, HIGH_SEL)):
    """A filter / projection shape in the plain, coalesced and high_sel forms."""
    for bit in forms:
        try:
            line(name + {0: "", BATCHED: " [batched]", HIGH_SEL: " [high_sel]"}[bit],
                 jit_check(schema, pred, projs, flags | bit))
        except ExecutionError as e:  # the front end's own refusal
            line(name, (-1, -1, "", e.message))
            return


def aggs(name, schema, pred, fns, flags, key=None):
    for bit in (0, BATCHED):
        tag = name + (" [batched]" if bit else "")
        if key is None:
            line(tag, _agg_jit(schema, pred, fns, flags | bit, compile_=False))
        else:
            line(tag, _grouped_jit(schema, pred, key, fns, flags | bit, compile_=False))


# --------------------------------------------------------------- the corpus
def compose():
    for sd in cc.SEEDS + cc.SMALL_SEEDS:
        filt("compose %d" % sd, cc.SCHEMA, *cc.gen_query(sd), flags=cc.FL)
    for sd in cc.SUBTILE_SEEDS:
        filt("compose subtile %d" % sd, cc.SCHEMA, *cc.subtile_query(sd), flags=cc.FL)
    with env(DFMI_NUMERIC_SUBTILES=4):
        for sd in cc.SEEDS + cc.SUBTILE_SEEDS:
            q = cc.gen_query(sd) if sd in cc.SEEDS else cc.subtile_query(sd)
            filt("compose %d forced M=4" % sd, cc.SCHEMA, *q, flags=cc.FL, forms=(0,))
        pred, chain = cc.literal_chain()
        filt("compose literal chain M=4", cc.SCHEMA, pred, [chain, Column(cc.X)], flags=cc.FL, forms=(0,))
    pred, chain = cc.literal_chain()
    filt("compose literal chain", cc.SCHEMA, pred, [chain, Column(cc.X)], flags=cc.FL)
    for sd in cc.AGG_SEEDS + cc.AGG_SUBTILE_SEEDS:
        pred, tree = cc.gen_numeric_tree(sd, subtile=sd in cc.AGG_SUBTILE_SEEDS)
        aggs("compose agg %d" % sd, cc.SCHEMA, pred, cc.aggregates_of(tree), cc.FLA)
        with env(DFMI_AGG_SUBTILES=4):
            aggs("compose agg %d M=4" % sd, cc.SCHEMA, pred, cc.aggregates_of(tree), cc.FLA)
    for sd in cc.GROUP_SEEDS:
        pred, key = cc.gen_group_key(sd, sd % 2 == 0)
        filt("compose group key %d" % sd, cc.SCHEMA, pred, [key], flags=cc.FL)
        if sd % 2 == 0:
            aggs("compose grouped %d" % sd, cc.SCHEMA, pred, cc.aggregates_of(Column(cc.X)), cc.FLA, key=key)
    for sd in cc.ORDER_SEEDS:
        filt("compose order key %d" % sd, cc.SCHEMA, None, [cc.order_key(sd)], flags=cc.FL)


def jit_cpu():
    filt("c2", F3, *c2_query())
    e = BinaryExpr(BinaryExpr(Column(0), Operator.Multiply, Column(1)), Operator.Gt, Column(4))
    filt("projection only", S, None, [e, Column(2), BinaryExpr(Column(0), Operator.Divide, Column(0))])
    sch = Schema([Field("c%d" % i, DataType.Utf8, False) for i in range(11)] + [Field("x", DataType.Float64, False)])
    filt("11 utf8 columns", sch, BinaryExpr(Column(11), Operator.Gt, Literal(Float64(0.5))), [])
    pred = BinaryExpr(BinaryExpr(Column(2), Operator.Eq, Literal(Utf8("w17"))), Operator.Or,
                      BinaryExpr(Column(2), Operator.NotEq, Column(2)))
    filt("utf8 compare", S, pred, [Column(2), Column(1)], _abi.DFMI_FLAG_EXT_UTF8_COMPARE)
    for t in NARROW:
        sch = Schema([Field("x", t, True), Field("y", t, False), Field("z", DataType.Float64, False)])
        lit = Literal(ScalarValue(t, 2.5 if t == DataType.Float32 else 3))
        pred = BinaryExpr(BinaryExpr(BinaryExpr(Column(0), Operator.Divide, Column(1)), Operator.Lt, lit), Operator.Or,
                          BinaryExpr(Column(0), Operator.GtEq, Column(1)))
        projs = [Column(0), BinaryExpr(BinaryExpr(Column(0), Operator.Multiply, Column(1)), Operator.Minus, lit),
                 Column(2)]
        filt("narrow %s" % t.name, sch, pred, projs, GA)
        filt("narrow %s projection" % t.name, sch, None, projs[1:] + [BinaryExpr(Column(0), Operator.Eq, lit)])
    types = [DataType.Int8, DataType.UInt16, DataType.Int32, DataType.UInt64, DataType.Float32, DataType.Float64]
    sch = Schema([Field("x%d" % i, t, True) for i, t in enumerate(types)] + [Field("s", DataType.Utf8, True)])
    fl = _abi.DFMI_FLAG_EXT_CAST | _abi.DFMI_FLAG_EXT_IS_NULL | GA
    projs = [Cast(Column(i), u) for i in range(len(types)) for u in types[:2]]
    filt("casts projection", sch, None, projs[:12], fl)
    pred = BinaryExpr(IsNull(Column(6)), Operator.Or,
                      BinaryExpr(Cast(Column(4), DataType.Int64), Operator.Gt, Cast(Column(0), DataType.Int64)))
    filt("cast / is null predicate", sch, pred, [IsNotNull(Column(1)), Cast(Column(5), DataType.UInt8)], fl)
    e = BinaryExpr(BinaryExpr(Column(0), Operator.Lt, Literal(Int64(3))), Operator.And,
                   BinaryExpr(Column(1), Operator.GtEq, Column(4)))
    div = BinaryExpr(Column(4), Operator.Divide, Column(1))
    for m in (2, 8):
        with env(DFMI_NUMERIC_SUBTILES=m):
            filt("c2 M=%d" % m, F3, *c2_query(), forms=(0,))
            filt("nullable M=%d utf8 out" % m, S, e, [div, Column(1), Column(2)], forms=(0,))
            filt("nullable M=%d" % m, S, e, [div, Column(1)], forms=(0,))
    rng = random.Random(7)
    for i in range(600):  # tests/test_jit_cpu.py test_random_shapes_generate_and_sample_compiles
        try:
            pred = tj._coerced(tj._rand_expr(rng, rng.randrange(1, 4), True))
            projs = [tj._coerced(tj._rand_expr(rng, rng.randrange(0, 3))) for _ in range(rng.randrange(0, 4))]
            compile_scalar_expr(None, pred, S)
            for p in projs:
                compile_scalar_expr(None, p, S)
        except ExecutionError:
            continue
        filt("random 7/%d" % i, S, pred, projs, forms=(0, BATCHED))


def utf8_order():
    for name, (pred, projs) in tu.SHAPES.items():
        filt("utf8 order %s" % name, tu.S, pred, projs, tu.BOTH)
    for op in tu.ORDER_OPS:
        forms = [BinaryExpr(Column(0), op, tu.lit(b"w2")), BinaryExpr(tu.lit(b"w2"), op, Column(1)),
                 BinaryExpr(Column(0), op, Column(1)), BinaryExpr(tu.lit(b"a"), op, tu.lit(b"b"))]
        for j, e in enumerate(forms):
            filt("utf8 order %s form %d" % (op.name, j), tu.S, e, [Column(2)], tu.BOTH, forms=(0,))
        filt("utf8 order %s without the flag" % op.name, tu.S, forms[0], [Column(2)], tu.CMP, forms=(0,))
    for op in (Operator.Eq, Operator.NotEq):  # Utf8 equality: column/column, column/literal, literal/literal
        for j, (l, r) in enumerate([(Column(0), Column(1)), (Column(0), tu.lit(b"w17")), (tu.lit(b"w17"), Column(1)),
                                    (tu.lit(b"a"), tu.lit(b"b"))]):
            filt("utf8 %s form %d" % (op.name, j), tu.S, BinaryExpr(l, op, r), [Column(0), Column(2)], tu.BOTH)
            filt("utf8 %s form %d projected" % (op.name, j), tu.S, None, [BinaryExpr(l, op, r), Column(2)], tu.BOTH,
                 forms=(0, BATCHED))
    for h, pre in ((8, 1), (8, 0), (4, 0)):
        with env(DFMI_UTF8_ORD_H=h, DFMI_UTF8_ORD_PRE=pre):
            filt("utf8 order range h=%d pre=%d" % (h, pre), tu.S, tu.range_pred(), [Column(0), Column(2)], tu.BOTH)
    for n in (0, 1, 4, 5, 8, 9, 200):
        a = bytes(97 + i % 26 for i in range(n))
        filt("utf8 order literal of %d bytes" % n, tu.S, BinaryExpr(Column(0), Operator.Lt, tu.lit(a)),
             [Column(0), Column(2)], tu.BOTH, forms=(0,))
    over = BinaryExpr(BinaryExpr(Column(0), Operator.Lt, tu.lit(b"x" * 200)), Operator.And,
                      BinaryExpr(Column(0), Operator.Gt, tu.lit(b"y" * 57)))
    filt("utf8 order literal pool over", tu.S, over, [Column(2)], tu.BOTH, forms=(0,))


def modulus_shapes():
    mod, MOD = tmod.mod, tmod.MOD
    s = Schema([Field("a", DataType.Int64, True), Field("b", DataType.Int64, False), Field("c", DataType.Int64, True)])
    pred = BinaryExpr(mod(Column(0), Column(1)), Operator.Eq, Literal(Int64(3)))
    filt("modulus column divisor", s, pred, [Column(2), mod(Column(2), Column(0))], MOD | 1)
    for t in (DataType.Int64, DataType.Int32):
        s = Schema([Field("k", t, False), Field("v", DataType.Float64, True)])
        pred = BinaryExpr(mod(Column(0), Literal(ScalarValue(t, 10))), Operator.Eq, Literal(ScalarValue(t, 3)))
        filt("modulus literal divisor %s" % t.name, s, pred, [Column(0), Column(1)], MOD | 1)
    for i, t in enumerate(tmod.TYPES):
        lit = Literal(ScalarValue(t, 2.5 if t in (DataType.Float32, DataType.Float64) else 7))
        filt("modulus projection %s" % t.name, tmod.S, None,
             [mod(Column(i), Column(i)), mod(Column(i), lit), mod(lit, Column(i))], MOD, forms=(0, BATCHED))
    s = Schema([Field("x", DataType.Float64, True), Field("y", DataType.Float64, False)])
    pred = BinaryExpr(mod(Column(0), Cast(Literal(Int64(2)), DataType.Float64)), Operator.Lt, Literal(Float64(0.5)))
    filt("modulus float literal divisor", s, pred, [Column(1), mod(Column(1), Literal(Float64(2.5)))], MOD)
    s = Schema([Field("k", DataType.Int64, False)])
    projs = [mod(Column(0), Literal(Int64(3 + j))) for j in range(16)]
    filt("modulus 32 literal slots", s, None, projs, MOD, forms=(0,))
    filt("modulus 33 literal slots", s, None, projs[:15] + [BinaryExpr(projs[15], Operator.Plus, Literal(Int64(1)))],
         MOD, forms=(0,))
    filt("modulus mixed operands", tmod.S, None, [mod(Column(3), Column(9))], MOD, forms=(0,))


def scalar_fn():
    fn, FN = tf.fn, tf.FN
    f3 = Schema([Field(c, DataType.Float64, c != "b") for c in "abc"])
    pred = BinaryExpr(BinaryExpr(fn("sqrt", Column(0)), Operator.Lt, Literal(Float64(0.5))), Operator.And,
                      BinaryExpr(fn("floor", BinaryExpr(Column(1), Operator.Multiply, Literal(Float64(10.0)))),
                                 Operator.GtEq, Literal(Float64(3.0))))
    filt("functions predicate", f3, pred, [fn("round", Column(2)), fn("mod", Column(0), Literal(Float64(3.0))),
                                           Column(1)], FN)
    g = Schema([Field("x", DataType.Float32, True), Field("y", DataType.Float32, False)])
    projs = [fn(nm, *[Column(0), Column(1)][:n], rt=DataType.Float32) for nm, n in sorted(tf.NAMES.items())]
    filt("functions float32 projection", g, None, projs, FN, forms=(0, BATCHED))


def cast_any():
    US, BOTH, TARGETS, NUMERIC = ta.US, ta.BOTH, ta.TARGETS, ta.NUMERIC
    filt("cast any projection", US, None, [Cast(Column(0), t) for t in TARGETS], BOTH, forms=(0, BATCHED))
    projs = [Cast(Column(2), t) for t in NUMERIC] + [
        Cast(Column(3), DataType.Boolean), Cast(Column(1), DataType.Boolean),
        Cast(BinaryExpr(Column(3), Operator.Gt, Literal(Float64(0.5))), DataType.Int64)]
    filt("cast any boolean casts", US, None, projs, BOTH, forms=(0, BATCHED))
    projs = [Column(1), Cast(Column(0), DataType.Int64), Cast(Column(0), DataType.Float32)]
    filt("cast any predicate", US, ta.all_targets_predicate(), projs, BOTH)
    flags = BOTH | AGG | GA
    fns = [AggregateFunction("SUM", (Cast(Column(0), t),), t) for t in NUMERIC]
    fns += [AggregateFunction("COUNT", (Cast(Column(0), DataType.Boolean),), DataType.UInt64),
            AggregateFunction("SUM", (Cast(Column(2), DataType.Int32),), DataType.Int32),
            AggregateFunction("SUM", (Cast(BinaryExpr(Column(3), Operator.Gt, Literal(Float64(0.5))), DataType.Int64),),
                              DataType.Int64)]
    gf = [AggregateFunction("SUM", (Cast(Column(0), DataType.Float64),), DataType.Float64),
          AggregateFunction("SUM", (Cast(Column(2), DataType.Int32),), DataType.Int32)]
    for pred in (None, ta.below(DataType.Float64)):
        tag = " with a predicate" if pred is not None else ""
        aggs("cast any aggregate arguments" + tag, US, pred, fns, flags)
        aggs("cast any grouped by a parsed key" + tag, US, pred, gf, flags, key=Cast(Column(0), DataType.Int64))


def aggregates():
    s = Schema([Field("q", DataType.Float64, False), Field("p", DataType.Float64, False),
                Field("d", DataType.Float64, False), Field("i", DataType.Int32, True),
                Field("f", DataType.Float32, True), Field("u", DataType.Utf8, True)])
    pred = BinaryExpr(BinaryExpr(Column(0), Operator.Lt, Literal(Float64(24.0))), Operator.And,
                      BinaryExpr(Column(2), Operator.GtEq, Literal(Float64(0.05))))
    q6 = [agg("SUM", BinaryExpr(Column(1), Operator.Multiply, Column(2)), s)]
    allf = [agg(f, Column(c), s) for f in ("SUM", "MIN", "MAX", "COUNT") for c in (3, 4)] + [agg("COUNT", Column(5), s)]
    avg = _abi.DFMI_FLAG_EXT_AGG_AVG if hasattr(_abi, "DFMI_FLAG_EXT_AGG_AVG") else 0
    for knobs in ({}, {"DFMI_AGG_SUBTILES": 4}, {"DFMI_AGG_SUBTILES": 2, "DFMI_ROWS_PER_THREAD": 4},
                  {"DFMI_PROJ_DENSE": 1}, {"DFMI_ROWS_PER_THREAD": 4}):
        tag = "".join(" %s=%s" % (k[5:], v) for k, v in knobs.items())
        with env(**knobs):
            aggs("q6" + tag, s, pred, q6, AGG | GA)
            aggs("every aggregate" + tag, s, None, allf, AGG)
            aggs("every aggregate with a predicate" + tag, s, pred, allf, AGG | GA)
            if avg:
                aggs("avg" + tag, s, pred, [agg("AVG", Column(c), s) for c in (0, 4)], AGG | GA | avg)
    g = Schema([Field("k", DataType.Boolean, True), Field("i", DataType.Int16, True),
                Field("x", DataType.Float64, True), Field("f", DataType.Float32, False)])
    gp = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.7)))
    fns = [agg("SUM", Column(2), g), agg("MIN", Column(3), g), agg("COUNT", Column(1), g), agg("MAX", Column(1), g)]
    for key in (0, 1):
        for p in (None, gp):
            for knobs in ({}, {"DFMI_PROJ_DENSE": 1}, {"DFMI_ROWS_PER_THREAD": 4}):
                with env(**knobs):
                    aggs("grouped key %d%s%s" % (key, " with a predicate" if p is not None else "",
                                                 "".join(" %s=%s" % (k[5:], v) for k, v in knobs.items())),
                         g, p, fns, AGG, key=Column(key))
    s = tb._schema()
    pred, fns = tb._queries(s)
    for p in (None, pred):
        tag = " with a predicate" if p is not None else ""
        aggs("agg batches" + tag, s, p, fns, AGG | GA)
        for key in (0, 3):
            aggs("agg batches grouped key %d%s" % (key, tag), s, p, fns, AGG | GA, key=Column(key))
    fl = tm.ANY | GA
    e = BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5)))
    fns = [agg("MIN", Column(0), tm.S), agg("max", Column(0), tm.S), agg("SUM", Column(2), tm.S),
           agg("COUNT", Column(0), tm.S), agg("MIN", e, tm.S), agg("MAX", Column(3), tm.S)]
    with_s = [agg("MIN", Column(1), tm.S), agg("SUM", Column(2), tm.S), agg("MAX", Column(1), tm.S)]
    for p in (None, gp):
        tag = " with a predicate" if p is not None else ""
        aggs("boolean extremes" + tag, tm.S, p, fns, fl)
        aggs("utf8 extremes" + tag, tm.S, p, with_s, fl)
        for key in (3, 4):
            aggs("boolean extremes grouped key %d%s" % (key, tag), tm.S, p, fns, fl, key=Column(key))


# every diagnostic knob the plan builder reads (exec_plan.cpp apply_diag_knobs), at
# non-default values, each over the base shapes below
KNOBS = [
    {"DFMI_ROWS_PER_THREAD": 4}, {"DFMI_BLOCK": 256}, {"DFMI_WAVES_PER_EU": 4}, {"DFMI_LOOKBACK_R": 2},
    {"DFMI_LOOKBACK_SLEEP": 8}, {"DFMI_LOOKBACK_SPREAD": 8}, {"DFMI_LOOKBACK_W": 16},
    {"DFMI_NT": 1}, {"DFMI_NT": 2}, {"DFMI_NT": 3}, {"DFMI_UTF8_PRESTAGE": 1}, {"DFMI_UTF8_PRESTAGE": 2},
    {"DFMI_GATHER_PHASES": 1}] + [{"DFMI_UTF8_GATHER": g} for g in range(7)] + [
    {"DFMI_UTF8_GATHER": 6, "DFMI_UTF8_DIRECT_GROUP": 4}, {"DFMI_UTF8_GATHER": 6, "DFMI_UTF8_DIRECT_GROUP": 1},
    {"DFMI_LATE_PROJ": 1}, {"DFMI_PROJ_DENSE": 1}, {"DFMI_TICKET": 1}, {"DFMI_UTF8_EARLY": 1},
    {"DFMI_LIGHT_COPY": 0}, {"DFMI_LONG_COPY": 1}, {"DFMI_LONG_COPY": 2}, {"DFMI_LIGHT_COPY": 0, "DFMI_LONG_COPY": 2},
    {"DFMI_UTF8_EQ_DENSE": 64}, {"DFMI_UTF8_EQ_REG": 2}, {"DFMI_UTF8_ORD_H": 8}, {"DFMI_UTF8_ORD_PRE": 0},
    {"DFMI_UTF8_RING": 1}, {"DFMI_UTF8_RING": 48}, {"DFMI_SUBTILES": 1}, {"DFMI_SUBTILES": 4},
    {"DFMI_NUMERIC_SUBTILES": 2}, {"DFMI_NUMERIC_SUBTILES": 4}, {"DFMI_NUMERIC_SUBTILES": 8},
    {"DFMI_NUMERIC_SUBTILES": 4, "DFMI_OUT_SLICES": 1}, {"DFMI_NUMERIC_SUBTILES": 4, "DFMI_OUT_SLICES": 4},
    {"DFMI_SUBTILES": 4, "DFMI_OUT_SLICES": 2}, {"DFMI_SUBTILE_PREFETCH": 0}, {"DFMI_SUBTILE_PREFETCH": 1},
    {"DFMI_SUBTILE_SPARSE": 0}, {"DFMI_NUMERIC_SUBTILES": 4, "DFMI_SUBTILE_SPARSE": 0},
    {"DFMI_UTF8_ARENA": 256}, {"DFMI_UTF8_ARENA": 256, "DFMI_UTF8_DBUF": 1},
    {"DFMI_UTF8_GATHER": 4, "DFMI_UTF8_IMAGE": 64}, {"DFMI_UTF8_GATHER": 4, "DFMI_UTF8_ST16": 1},
    {"DFMI_UTF8_GATHER": 4, "DFMI_UTF8_PAIRS": 1}, {"DFMI_UTF8_GATHER": 4, "DFMI_UTF8_ARENA": 256, "DFMI_UTF8_DBUF": 1},
    {"DFMI_UTF8_GATHER": 5, "DFMI_UTF8_PRESTAGE": 1, "DFMI_UTF8_EARLY": 1},
]


def knob_bases():
    lt = BinaryExpr(Column(1), Operator.Lt, Literal(Float64(0.5)))
    eq = BinaryExpr(Column(0), Operator.Eq, Literal(Utf8("w17dizjxms")))
    two = Schema([Field("s", DataType.Utf8, True), Field("t", DataType.Utf8, False), Field("v", DataType.Float64, True)])
    return [("c2", F3, *c2_query(), 0), ("c3lt", C3, lt, [Column(0), Column(1)], 2), ("c3eq", C3, eq, [Column(0), Column(1)], 2),
            ("range", tu.S, tu.range_pred(), [Column(0), Column(2)], tu.BOTH),
            ("mixed", two, BinaryExpr(BinaryExpr(Column(2), Operator.Lt, Literal(Float64(0.5))), Operator.And,
                                      BinaryExpr(Column(0), Operator.NotEq, Literal(Utf8("abc")))),
             [Column(0), Column(1), BinaryExpr(Column(2), Operator.Plus, Column(2))], tu.BOTH),
            ("nullable out", S, BinaryExpr(Column(0), Operator.Lt, Literal(Int64(3))),
             [Cast(Column(1), DataType.Int32), Column(3)], _abi.DFMI_FLAG_EXT_CAST | GA),
            ("project", S, None, [BinaryExpr(Column(0), Operator.Divide, Column(0)), Column(3)], 0)]


def knobs():
    for name, schema, pred, projs, flags in knob_bases():
        filt("base " + name, schema, pred, projs, flags)
        for kv in KNOBS:
            with env(**kv):
                filt("base %s%s" % (name, "".join(" %s=%s" % (k[5:], v) for k, v in kv.items())), schema, pred, projs,
                     flags, forms=(0, BATCHED))


def rem_literal_child():
    """DFMI_REM_LITERAL is read once per process: the parent starts this."""
    mod, MOD = tmod.mod, tmod.MOD
    for t in (DataType.Int64, DataType.Int32, DataType.UInt8):
        s = Schema([Field("k", t, False), Field("v", DataType.Float64, True)])
        pred = BinaryExpr(mod(Column(0), Literal(ScalarValue(t, 10))), Operator.Eq, Literal(ScalarValue(t, 3)))
        filt("modulus literal divisor %s REM_LITERAL=0" % t.name, s, pred,
             [Column(0), mod(Column(0), Literal(ScalarValue(t, 7)))], MOD | 1)
    print("# %d" % COUNT)


def main():
    if sys.argv[1:] == ["--rem-literal-child"]:
        return rem_literal_child()
    for part in (compose, jit_cpu, utf8_order, modulus_shapes, scalar_fn, cast_any, aggregates, knobs):
        part()
    sys.stdout.flush()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--rem-literal-child"], check=True,
                           capture_output=True, text=True, env=dict(os.environ, DFMI_DIAG="1", DFMI_REM_LITERAL="0"))
    lines = child.stdout.splitlines()
    print("\n".join(lines[:-1]))
    print("# %d shapes" % (COUNT + int(lines[-1][2:])), file=sys.stderr)


if __name__ == "__main__":
    main()
