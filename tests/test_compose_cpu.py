"""Composed expressions across the extension families, the parts that need no
GPU (tests/compose_cases.py): the unified restatement pinned on each family's
own expectation, every seed of tests/test_gpu_compose.py checked for use, the
generator's coverage of node kinds and of cross-family (parent, child) pairs,
the planted errors of the error-order templates, and a sample of the generated
kernels compiled for gfx950."""
import numpy as np

import compose_cases as cc
import test_gpu_cast_any as ca
import test_gpu_modulus as gm
import test_gpu_scalar_fn as sf
import test_gpu_utf8_order as uo
from compose_cases import FAMILY, KINDS, UNARY
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Cast, Column, DataType, Float64, Int64, Literal, Operator
from test_gpu_cast_any import Str, Table
from test_jit_cpu import jit_check

F64, I64 = DataType.Float64, DataType.Int64


def same(got, want, what):
    """Two reference results, bit for bit on the valid slots."""
    if isinstance(got, Str):
        got = got.oracle_array()
    assert got.data_type == want.data_type and got.length == want.length, what
    assert got.null_count == want.null_count and np.array_equal(got.valid_mask(), want.valid_mask()), what
    ok = want.valid_mask()
    if want.data_type == DataType.Utf8:
        assert [g for g, v in zip(got.numpy_values(), ok) if v] == [w for w, v in zip(want.numpy_values(), ok) if v], what
        return
    g, w = np.ascontiguousarray(got.numpy_values()), np.ascontiguousarray(want.numpy_values())
    if want.data_type != DataType.Boolean:
        g, w = g.view("u%d" % g.dtype.itemsize), w.view("u%d" % w.dtype.itemsize)
    assert np.array_equal(g[ok], w[ok]), (what, np.flatnonzero((g != w) & ok)[:5])


def table_of(schema, batch):
    """A RecordBatch as the unified table model (Utf8: the raw bytes of null rows too)."""
    cols = [Str(c.numpy_values(), c.valid_mask()) if c.data_type == DataType.Utf8 else c for c in batch.columns]
    return Table(schema.fields, cols)


# ------------------------------------------------------------------- pinning
def test_pinned_on_the_cast_family():
    tab = ca.bool_table()
    halves = [[ca.cast(0, t) for t in ca.NUMERIC[:5]], [ca.cast(3 + i, ca.BOOL) for i in (0, 3, 8, 9)]]
    for pred in (None, ca.lt(Column(1), 0.5)):
        for projs in halves:
            for e, g, w in zip(projs, cc.expected(tab, pred, projs), ca.expected(tab, pred, projs)):
                same(g, w, (repr(pred), repr(e)))
    col, vals = ca.number_column(3000, 7, True)
    tab = Table([ca.Field("s", ca.U8, True), ca.Field("v", I64, False)],
                [col, ca.Array.from_numpy(I64, np.arange(3000, dtype=np.int64) * 3)])
    pred, projs = ca.lt(ca.cast(0, F64), float(np.quantile(vals, 0.5)) + 0.5), [Column(1), ca.cast(0, I64), ca.cast(0, F64)]
    want = ca.expected(tab, pred, projs)
    assert 1000 < want[0].length < 2000 and want[1].null_count > 0
    for g, w in zip(cc.expected(tab, pred, projs), want):
        same(g, w, "number column")


def test_pinned_on_the_function_family():
    s, b = sf.random_table(4097, 100)
    projs = [sf.fn(nm, Column(0)) for nm in sf.UNARY] + [sf.fn("mod", Column(1), Column(0)),
                                                          sf.fn("sqrt", BinaryExpr(Column(1), Operator.Plus, Column(2)))]
    pred = BinaryExpr(BinaryExpr(sf.fn("sqrt", Column(0)), Operator.Lt, Literal(Float64(0.5))), Operator.And,
                      BinaryExpr(sf.fn("floor", BinaryExpr(Column(1), Operator.Multiply, Cast(Literal(Int64(10)), F64))),
                                 Operator.GtEq, Cast(Literal(Int64(3)), F64)))
    for p in (None, pred):
        want = sf.expected(s, b, p, projs, sf.FLAGS_SQL)
        assert p is None or 0 < want[0].length < 4097
        for e, g, w in zip(projs, cc.expected(table_of(s, b), p, projs), want):
            same(g, w, (repr(p), repr(e)))


def test_pinned_on_the_modulus_family():
    s, b, k, v = gm.kv_table(4162, seed=13)
    pred, projs = gm.batch_forms_query()
    projs = projs + [gm.mod(gm.mod(Column(1), Column(0)), Literal(Int64(7)))]
    for p in (None, pred):
        want = gm.expected(s, b, p, projs)
        for e, g, w in zip(projs, cc.expected(table_of(s, b), p, projs), want):
            same(g, w, (repr(p), repr(e)))


def test_pinned_on_the_ordering_family():
    b = uo.table()
    tab = table_of(uo.S3, b)
    projs = [BinaryExpr(Column(0), Operator.Lt, uo.lit(b"abcd")), BinaryExpr(uo.lit(uo.L40), Operator.GtEq, Column(0)),
             BinaryExpr(Column(0), Operator.LtEq, Column(1)), Column(2)]
    mixed = BinaryExpr(uo.V_LT, Operator.And, BinaryExpr(Column(0), Operator.GtEq, uo.lit(b"abc")))
    for p in (None, uo.V_LT, mixed):
        want = uo.expected(uo.S3, b, p, projs)
        assert 0 < want[0].length <= b.num_rows()
        for e, g, w in zip(projs, cc.expected(tab, p, projs), want):
            same(g, w, (repr(p), repr(e)))
        for g, w in zip(cc.expected(tab, p, [Column(0)]), uo.expected(uo.S3, b, p, [Column(0)])):
            if p is not None:  # (the passed-through column: the bytes of the selected rows, null slots' too)
                assert g.strings == w.numpy_values()


# ------------------------------------------------------------ every seed usable
def generates(pred, projs, flags=cc.FL):
    for e in ([pred] if pred is not None else []) + list(projs):
        compile_scalar_expr(None, e, cc.SCHEMA, flags)
    rc, code, msg, src = jit_check(cc.SCHEMA, pred, projs, flags)
    assert rc > 0, (code, msg, repr(pred), [repr(p) for p in projs])  # (a program-limit refusal is a generator bug)
    return src


def test_the_generator_is_deterministic():
    for seed in cc.SEEDS[:20]:
        assert repr(cc.gen_query(seed)) == repr(cc.gen_query(seed))
    assert len({repr(cc.gen_query(seed)) for seed in cc.SEEDS}) == len(cc.SEEDS)


def queries():
    out = [(sd, cc.ROWS, cc.gen_query(sd)) for sd in cc.SEEDS] + [(sd, cc.ROWS_SMALL, cc.gen_query(sd)) for sd in cc.SMALL_SEEDS]
    return out + [(sd, cc.ROWS, cc.subtile_query(sd)) for sd in cc.SUBTILE_SEEDS]


def test_the_seed_lists_have_the_sizes_the_gpu_cases_take():
    assert len(cc.SEEDS) == 16 * 6 and len(cc.SMALL_SEEDS) == 6 and len(cc.AGG_SEEDS) == 12
    assert len(cc.GROUP_SEEDS) == 8 and len(cc.ORDER_SEEDS) == 8
    every = cc.SEEDS + cc.SMALL_SEEDS + cc.SUBTILE_SEEDS + cc.AGG_SEEDS + cc.AGG_SUBTILE_SEEDS + cc.GROUP_SEEDS + \
        cc.ORDER_SEEDS
    assert len(cc.AGG_SUBTILE_SEEDS) == 12
    assert len(set(every)) == len(every)


def test_every_filter_project_seed_is_usable(monkeypatch):
    """Compiles, generates source (in the forced sub-tile form too), has an
    expected value and raises nothing; deterministic; within the limits."""
    plain = {}
    for seed, n, (pred, projs) in queries():
        assert 1 <= len(projs) <= min(4, cc.MAX_OUTPUTS)
        plain[seed] = generates(pred, projs)
        tab = cc.value_table(n)
        want = cc.expected(tab, pred, projs)
        assert len(want) == len(projs) and cc.first_error(tab, pred, projs) is None, seed
        for t in cc.split_table(cc.value_table(), [1, 64, 4044, 0]) if n == cc.ROWS else []:
            assert cc.first_error(t, pred, projs) is None, seed
    assert sum(1 for _, _, (pred, _) in queries()[:102] if pred is None) in range(15, 40)  # about one in four
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_NUMERIC_SUBTILES", "4")
    forced = {seed: generates(pred, projs) for seed, n, (pred, projs) in queries()}
    # every Utf8-free seed, and a few of the others, take the sub-tile form
    assert all(forced[sd] != plain[sd] for sd in cc.SUBTILE_SEEDS)
    takes = [sd for sd in cc.SEEDS if cc.takes_subtile_form(*cc.gen_query(sd))]
    assert takes == [sd for sd in cc.SEEDS if forced[sd] != plain[sd]] and len(takes) >= 5


def test_a_literal_takes_one_slot_in_every_form(monkeypatch):
    """17 literals in a projection and one in the predicate generate in the
    plain and in the forced sub-tile form of the filtered kernel (the
    aggregate kernel's forms: tests/test_gpu_compose.py)."""
    pred, chain = cc.literal_chain()
    assert cc.takes_subtile_form(pred, [chain]) and cc.takes_agg_subtile_form(pred, chain)
    plain = generates(pred, [chain, Column(cc.X)])
    assert "A.lits[17]" in plain and "A.lits[18]" not in plain
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_NUMERIC_SUBTILES", "4")
    forced = generates(pred, [chain, Column(cc.X)])
    assert forced != plain and "A.lits[17]" in forced and "A.lits[18]" not in forced


def test_every_aggregate_group_and_order_seed_is_usable():
    tab = cc.value_table()
    for seed in cc.AGG_SEEDS:
        pred, tree = cc.gen_numeric_tree(seed)
        generates(pred, [tree])
        for a in cc.aggregates_of(tree):
            compile_expr(None, a, cc.SCHEMA, cc.FLA)
        assert cc.first_error(tab, pred, [tree]) is None, seed
    for seed in cc.AGG_SUBTILE_SEEDS:
        pred, tree = cc.gen_numeric_tree(seed, subtile=True)
        generates(pred, [tree])
        for a in cc.aggregates_of(tree):
            compile_expr(None, a, cc.SCHEMA, cc.FLA)
        assert cc.takes_agg_subtile_form(pred, tree) and cc.first_error(tab, pred, [tree]) is None, seed
    assert [sd for sd in cc.AGG_SEEDS if cc.takes_agg_subtile_form(*cc.gen_numeric_tree(sd))] == []  # (hence the list above)
    for seed in cc.GROUP_SEEDS:
        pred, key = cc.gen_group_key(seed, seed % 2 == 0)
        generates(pred, [key])
        assert key.get_type(cc.SCHEMA) == (I64 if seed % 2 == 0 else F64)
        assert cc.first_error(tab, pred, [key]) is None, seed
        (k,) = cc.expected(tab, pred, [key])
        distinct = set(np.array(k.numpy_values())[k.valid_mask()].view(np.uint64).tolist())
        assert 4 <= len(distinct) <= 64, (seed, len(distinct))
        if seed % 2 == 0:  # within 16 consecutive values: the fused key window
            assert distinct <= set(range(16)), seed
    for seed in cc.ORDER_SEEDS:
        key = cc.order_key(seed)
        generates(None, [key])
        assert cc.first_error(tab, None, [key]) is None, seed


# -------------------------------------------------------------------- coverage
NUMERIC_PARENTS = ["mod_lit", "mod_col", "cast_num_bool", "fn_mod"] + ["fn_" + nm for nm in UNARY]
NUMERIC_CHILDREN = ["mod_lit", "mod_col", "fn_mod", "cast_utf8_int", "cast_utf8_float", "cast_bool_num"] + \
    ["fn_" + nm for nm in UNARY]
BOOLEAN_CHILDREN = ["cast_utf8_bool", "cast_num_bool", "ord_lit", "ord_col"]


def impossible(parent, child):
    """Why a (parent kind, child kind) pair of two families cannot be built.
    (compose_cases.py, "node kinds", names what the matrix does not require:
    pairs inside the cast family, and which operand the child is.)"""
    if parent.startswith("cast_utf8"):
        return "CAST from Utf8 takes a column only"
    if parent.startswith("ord_"):
        return "an ordering comparison takes Utf8 columns and literals only"
    if parent == "cast_bool_num":
        return None if child in BOOLEAN_CHILDREN else "CAST from Boolean takes a Boolean child"
    assert parent in NUMERIC_PARENTS
    return None if child in NUMERIC_CHILDREN else "a numeric operand: no Boolean child"


def test_coverage_of_node_kinds_and_cross_family_pairs():
    kinds, pairs = {}, set()
    for seed in cc.SEEDS + cc.SMALL_SEEDS:
        pred, projs = cc.gen_query(seed)
        for e in ([pred] if pred is not None else []) + projs:
            cc.kinds_and_pairs(e, kinds, pairs)
    assert set(kinds) == set(KINDS)
    assert not [(k, kinds[k]) for k in KINDS if kinds[k] < 10]
    cross = [(p, c) for p in FAMILY for c in FAMILY if FAMILY[p] != FAMILY[c]]
    possible = [pc for pc in cross if impossible(*pc) is None]
    assert len(cross) == 174 and len(possible) == 66
    assert not [pc for pc in possible if pc not in pairs]
    assert not [pc for pc in cross if impossible(*pc) and pc in pairs]  # (the list of impossible pairs is right)


# ----------------------------------------------------------------- error order
def test_error_templates_plant_the_error_they_name():
    cases = cc.error_cases()
    assert len(cases) == 12 and len({c[0] for c in cases}) == 12
    for name, tab, pred, projs, planted in cases:
        assert cc.first_error(tab, pred, projs) == planted, name
        if planted != cc.MATH_OPS:
            for e in ([pred] if pred is not None else []) + list(projs):
                compile_scalar_expr(None, e, tab.schema, cc.FL)
        if planted is None:
            (r, _) = cc.expected(tab, pred, projs)
            assert not r.valid_mask()[[7, 8, 4100]].any() and r.valid_mask()[9:4100].all()
    planted = {c[4] for c in cases}
    assert planted == {cc.DIV0, cc.DIV_OVERFLOW, cc.REM_OVERFLOW, cc.MATH_OPS, cc.limit_error(F64), None}


# -------------------------------------------------------------- compile sample
def test_a_sample_of_the_generated_kernels_compiles_for_gfx950():
    seen = set()
    for seed in cc.SEEDS[::8] + cc.SUBTILE_SEEDS[:2]:
        pred, projs = cc.gen_query(seed) if seed in cc.SEEDS else cc.subtile_query(seed)
        src = generates(pred, projs)
        if src in seen or len(seen) >= 12:
            continue
        seen.add(src)
        rc, code, msg, _ = jit_check(cc.SCHEMA, pred, projs, cc.FL, compile_=True)
        assert rc > 0, (seed, msg, repr(pred), [repr(p) for p in projs])
    assert len(seen) >= 10
