"""Composed expressions across the extension families: one restatement and one
generator for tests/test_compose_cpu.py and tests/test_gpu_compose.py.

The oracle executes the base operators, numeric CAST, IS NULL and Utf8 `=`.
Every other node kind has a restatement in the test file of its own family:
Modulus (test_modulus_cpu.restate), the scalar functions
(test_gpu_scalar_fn.restate), CAST of a Utf8 column (test_cast_any_cpu.restate
through Str.parsed), Boolean <-> numeric casts (test_gpu_cast_any.lower) and
the Utf8 ordering comparisons (test_gpu_utf8_order: Python's bytes order and
arrow's cmp_opt). `lower` here works bottom-up over a whole tree: each
extension node's children are evaluated through the oracle on the table
lowered so far, the family's restatement is applied, the result is appended as
a materialised nullable column and the node becomes that Column. No arithmetic
is written here.

The table model is test_gpu_cast_any's (`Str`, `Table`): a null Utf8 row keeps
its bytes, and a Selection's output is all-valid with the bytes and the raw
value slots as they are (filter.rs:84-93).

`gen_query(seed)` builds typed trees of depth <= 4 over one fixed schema with
the casts the planner would insert, inside the program limits; `value_table`
holds data on which no generated node raises. `first_error` restates the
reference's error order for the hand-written templates of
`error_cases`."""
import random

import numpy as np

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, np_dtype
from datafusion_amd.logicalplan import (AggregateFunction, BinaryExpr, Cast, Column, DataType, Float64, Int64, IsNotNull,
                                        IsNull, Literal, Operator, PlanError, ScalarFunction, ScalarValue,
                                        binary_expr_coerced)
from oracle_ffi import oracle_filter_project
from test_cast_any_cpu import CORPUS, LIMIT_STRING, limit_message, random_strings
from test_gpu_cast_any import Str, Table
from test_gpu_scalar_fn import restate as restate_fn
from test_gpu_utf8_order import DICT, ORDER_OPS, cmp_opt, lit as str_lit, lit_bytes, order_values
from test_modulus_cpu import restate as restate_mod

T = DataType
U8, BOOL, I64, I32, I8, U64, F64, F32 = T.Utf8, T.Boolean, T.Int64, T.Int32, T.Int8, T.UInt64, T.Float64, T.Float32
SIGNED = (T.Int8, T.Int16, T.Int32, T.Int64)
INTS = SIGNED + (T.UInt8, T.UInt16, T.UInt32, T.UInt64)
FLOATS = (F32, F64)
NUMERIC = INTS + FLOATS

MOD, FN, ANY, ORD = (_abi.DFMI_FLAG_EXT_MODULUS, _abi.DFMI_FLAG_EXT_SCALAR_FUNCTIONS, _abi.DFMI_FLAG_EXT_CAST_ANY,
                     _abi.DFMI_FLAG_EXT_UTF8_ORDER)
EXT = MOD | FN | ANY | ORD  # what `lower` removes from a tree
FL = EXT | _abi.DFMI_FLAG_EXT_GATHER_ALL | _abi.DFMI_FLAG_EXT_UTF8_COMPARE | _abi.DFMI_FLAG_EXT_CAST | \
    _abi.DFMI_FLAG_EXT_IS_NULL
FLA = FL | _abi.DFMI_FLAG_EXT_AGGREGATE
FLS = FL | _abi.DFMI_FLAG_EXT_SORT

MATH = (Operator.Plus, Operator.Minus, Operator.Multiply, Operator.Divide, Operator.Modulus)
CMP = (Operator.Eq, Operator.NotEq, Operator.Lt, Operator.LtEq, Operator.Gt, Operator.GtEq)
UNARY = ["sqrt", "abs", "floor", "ceil", "round", "trunc"]

DIV0 = ("ArrowError(DivideByZero)", "DivideByZero")
DIV_OVERFLOW = ("panic", "attempt to divide with overflow")
REM_OVERFLOW = ("panic", "attempt to calculate the remainder with overflow")
MATH_OPS = ("ExecutionError", "math_ops")


def limit_error(t):
    return ("NotImplemented", limit_message(t))


# ------------------------------------------------------------ the restatement
def type_of(e, tab):
    return e.get_type(tab.schema)


def oracle_project(tab, exprs):
    """Extension-free expressions over the table, through the oracle."""
    return [a for _, a in oracle_filter_project(tab.schema, tab.oracle_batch(), None, list(exprs), FL & ~EXT)]


def is_utf8_operand(e, tab):
    return (isinstance(e, Literal) and e.value.dtype == U8) or (isinstance(e, Column) and type_of(e, tab) == U8)


def utf8_operand(e, tab):
    n = tab.rows()
    if isinstance(e, Literal):
        return [lit_bytes(e)] * n, np.ones(n, bool)
    c = tab.cols[e.index]
    return c.strings, c.valid


def materialise(tab, t, vals, valid):
    vals = np.array(vals).copy()
    vals[~valid] = 0
    tab = tab.with_column(t, vals, valid)
    return Column(len(tab.fields) - 1), tab


def lower(e, tab):
    """(e', tab'): e with every extension node replaced by a Column of tab',
    which is tab with the restated columns appended."""
    if isinstance(e, (Column, Literal)):
        return e, tab
    if isinstance(e, ScalarFunction):
        args = []
        for a in e.args:
            a, tab = lower(a, tab)
            args.append(a)
        cols = oracle_project(tab, args)
        valid = np.ones(tab.rows(), bool)
        for c in cols:
            valid &= c.valid_mask()
        return materialise(tab, e.return_type, restate_fn(e.name, [np.array(c.numpy_values()) for c in cols]), valid)
    if isinstance(e, (IsNull, IsNotNull)):
        x, tab = lower(e.expr, tab)
        return type(e)(x), tab
    if isinstance(e, Cast):
        if isinstance(e.expr, Column) and type_of(e.expr, tab) == U8:
            vals, ok, lim = tab.cols[e.expr.index].parsed(e.data_type)
            assert not lim, "a row at the program limit: not an expected-value query"
            return materialise(tab, e.data_type, vals, ok)
        x, tab = lower(e.expr, tab)
        src_t = type_of(x, tab)
        if (src_t == BOOL) == (e.data_type == BOOL):
            return Cast(x, e.data_type), tab
        (src,) = oracle_project(tab, [x])
        if src_t == BOOL:  # true -> 1, false -> 0
            vals = np.array(src.numpy_values()).astype(bool).astype(np_dtype(e.data_type))
        else:  # x != 0: NaN true, -0.0 false
            vals = np.array(src.numpy_values()) != 0
        return materialise(tab, e.data_type, vals, src.valid_mask())
    assert isinstance(e, BinaryExpr), e
    if e.op in ORDER_OPS and is_utf8_operand(e.left, tab) and is_utf8_operand(e.right, tab):
        (a, av), (b, bv) = utf8_operand(e.left, tab), utf8_operand(e.right, tab)
        res = cmp_opt(e.op, np.asarray(av), np.asarray(bv), order_values(e.op, a, b))
        return materialise(tab, BOOL, res, np.ones(tab.rows(), bool))
    l, tab = lower(e.left, tab)
    r, tab = lower(e.right, tab)
    if e.op != Operator.Modulus:
        return BinaryExpr(l, e.op, r), tab
    a, b = oracle_project(tab, [l, r])
    valid = a.valid_mask() & b.valid_mask()
    y = np.array(b.numpy_values()).copy()
    y[~valid] = 1  # (a null row raises nothing)
    vals, zero, over = restate_mod(np.array(a.numpy_values()), y)
    assert not zero.any() and not over.any(), "a failing row: not an expected-value query"
    return materialise(tab, a.data_type, vals, valid)


def lower_all(exprs, tab):
    out = []
    for e in exprs:
        e, tab = lower(e, tab)
        out.append(e)
    return out, tab


def filtered(tab, pred):
    """The Selection's output: every column's selected rows, validity dropped."""
    if pred is None:
        return tab
    p, t2 = lower(pred, tab)
    n = tab.rows()
    t2 = t2.with_column(I64, np.arange(n, dtype=np.int64), np.ones(n, bool))
    keep = [i for i, f in enumerate(tab.fields) if f.data_type != U8]
    out = oracle_filter_project(t2.schema, t2.oracle_batch(), p, [Column(i) for i in keep] + [Column(len(t2.fields) - 1)],
                                FL & ~EXT)
    ids = np.array(out[-1][1].numpy_values())
    cols = [tab.cols[i].take(ids) if f.data_type == U8 else out[keep.index(i)][1] for i, f in enumerate(tab.fields)]
    return Table([Field(f.name, f.data_type, False) for f in tab.fields], cols)


def expected(tab, pred, projs):
    """Projection(Selection?(tab)): per projection an Array, or a Str for a passed-through Utf8 column."""
    ft = filtered(tab, pred)
    ps, t = lower_all(projs, ft)
    idx = [j for j, e in enumerate(projs) if type_of(e, ft) != U8]
    arrays = oracle_project(t, [ps[j] for j in idx]) if idx else []
    out = [ft.cols[e.index] if type_of(e, ft) == U8 else None for e in projs]
    for j, a in zip(idx, arrays):
        out[j] = a
    return out


def lowered_aggregates(tab, pred, aggs, keys=()):
    """(keys', aggs', tab') over the Selection's output, for the oracle's aggregate entry points."""
    ft = filtered(tab, pred)
    ks, t = lower_all(list(keys), ft)
    args, t = lower_all([a.args[0] for a in aggs], t)
    return ks, [AggregateFunction(a.name, (x,), a.return_type) for a, x in zip(aggs, args)], t


# ---------------------------------------------------------------- error order
def postfix(e):
    """The nodes of e, children first (the reference's evaluation order)."""
    if isinstance(e, BinaryExpr):
        return postfix(e.left) + postfix(e.right) + [e]
    if isinstance(e, ScalarFunction):
        return [x for a in e.args for x in postfix(a)] + [e]
    if isinstance(e, (Cast, IsNull, IsNotNull)):
        return postfix(e.expr) + [e]
    return [e]


def node_error(e, tab):
    """(kind, message) of node e's earliest failing row over tab, or None.
    Every node below e is clean, so its operands can be evaluated."""
    if isinstance(e, Cast) and e.data_type in FLOATS and isinstance(e.expr, Column) and type_of(e.expr, tab) == U8:
        return limit_error(e.data_type) if tab.cols[e.expr.index].parsed(e.data_type)[2] else None
    if not (isinstance(e, BinaryExpr) and e.op in MATH):
        return None
    lt, rt = type_of(e.left, tab), type_of(e.right, tab)
    if lt != rt or lt not in NUMERIC:
        return MATH_OPS  # static: whatever the rows are
    if e.op not in (Operator.Divide, Operator.Modulus):
        return None
    (l, r), t = lower_all([e.left, e.right], tab)
    a, b = oracle_project(t, [l, r])
    valid = a.valid_mask() & b.valid_mask()
    x, y = np.array(a.numpy_values()), np.array(b.numpy_values())
    zero = valid & (y == 0)  # (-0.0 too)
    over = np.zeros(len(x), bool)
    if lt in SIGNED:
        over = valid & (x == np.iinfo(x.dtype).min) & (y == -1)
    bad = np.flatnonzero(zero | over)
    if not len(bad):
        return None
    if zero[bad[0]]:
        return DIV0
    return DIV_OVERFLOW if e.op == Operator.Divide else REM_OVERFLOW


def first_error(tab, pred, projs):
    """The error the reference raises: the predicate's nodes in postfix order
    over every row, then each projection's over the selected rows; the first
    fallible node with a failing evaluated row decides, by its earliest row."""
    if pred is not None:
        for e in postfix(pred):
            err = node_error(e, tab)
            if err:
                return err
    ft = filtered(tab, pred)
    for p in projs:
        for e in postfix(p):
            err = node_error(e, ft)
            if err:
                return err
    return None


# ------------------------------------------------------------------- the data
COLS = [("a", I64, True), ("b", I64, False), ("c", I32, True), ("d", I8, True), ("e", U64, True), ("x", F64, True),
        ("y", F32, True), ("f", BOOL, True), ("s", U8, True), ("u", U8, True),
        # dedicated divisors: no 0 and no -1 in any slot, those of null rows included
        ("di", I64, True), ("d8", I8, False), ("dx", F64, True),
        ("i", I64, False)]  # the row index
A, B, C_, D, E, X, Y, F, S, U, DI, D8, DX, I = range(len(COLS))
FIELDS = [Field(n, t, nullable) for n, t, nullable in COLS]
EMPTY = Table(FIELDS, [])
SCHEMA = EMPTY.schema
NUM_COLS = [A, B, C_, D, E, X, Y, DI, D8, DX]
ROWS, ROWS_SMALL = 4097 + 12, 67  # more than one tile with a ragged tail; one partial tile

STRINGS = [s for s in CORPUS if s != LIMIT_STRING] + DICT + random_strings(160, 11, long_too=True)
# literals of the ordering and equality nodes: short ones (8 per program, 256 bytes in all)
STR_LITERALS = [b"", b"a", b"abcd", b"abcde", b"abcdefgh", b"abcdefghi", b"abcdefgh\x80", b"1", b"5", b"true", b"-1",
                b"007", b"m", b"\xff"]


def int_column(rng, t, n):
    info = np.iinfo(np_dtype(t))
    edges = [info.min, info.max, 0, 1, info.max - 1, info.min + 1, 2, 7, 16, 100] + ([-1, -2, -7] if info.min < 0 else [])
    body = (rng.integers(info.min, info.max, n, dtype=np_dtype(t), endpoint=True).astype(object) >>
            rng.integers(0, info.bits, n).astype(object)).astype(np_dtype(t))
    pick = rng.random(n) < 0.15
    body[pick] = np.array(edges, dtype=object)[rng.integers(0, len(edges), int(pick.sum()))].astype(np_dtype(t))
    body[:len(edges)] = np.array(edges, dtype=object).astype(np_dtype(t))
    return body


def float_column(rng, t, n):
    f = np_dtype(t)
    u = np.uint64 if t == F64 else np.uint32
    info = np.finfo(f)
    top, mb = info.bits - 1, info.nmant
    expo = ((1 << (top - mb)) - 1) << mb
    nans = [expo | (1 << (mb - 1)), expo | (1 << (mb - 1)) | 0x123, expo | 1, expo | 0x155]  # quiet, payloads, signalling
    nans += [b | (1 << top) for b in nans]
    edges = np.concatenate([np.array(nans, u).view(f),
                            np.array([0.0, -0.0, np.inf, -np.inf, info.tiny, -info.tiny, info.max, -info.max, 0.5, -0.5,
                                      1.0, -1.0, 2.5, -2.5, 2.0 ** mb, 2.0 ** 63, -2.0 ** 63, 1e9, 255.0, 127.5], f),
                            np.array([1, 3, (1 << mb) - 1, (1 << top) | 1], u).view(f)])  # subnormals
    body = ((rng.random(n) - 0.5) * 10.0 ** rng.integers(-3, 12, n)).astype(f)
    small = rng.random(n) < 0.4
    body[small] = rng.integers(-40, 40, int(small.sum())).astype(f) / f(4)  # halves and quarters: rounding ties
    pick = rng.random(n) < 0.15
    body[pick] = edges[rng.integers(0, len(edges), int(pick.sum()))]
    body[:len(edges)] = edges
    return body


_tables = {}


def value_table(n=ROWS, seed=5):
    """The fixed schema over n rows: edges first, about 20 % nulls in the
    nullable columns. Built once per (n, seed) and never changed."""
    if (n, seed) in _tables:
        return _tables[(n, seed)]
    rng = np.random.default_rng(seed)
    cols = []
    for name, t, nullable in COLS:
        valid = rng.random(n) >= 0.2 if nullable else np.ones(n, bool)
        if name in ("di", "d8"):
            v = rng.integers(2, 100, n) * rng.choice([-1, 1], n)
            v[:6] = [2, -2, 3, 16, 99, -99]
            col = Array.from_numpy(t, v.astype(np_dtype(t)), None if valid.all() else valid)
        elif name == "dx":
            v = (rng.integers(1, 400, n) / 8.0) * rng.choice([-1.0, 1.0], n)
            v[:6] = [0.125, -0.125, np.inf, -np.inf, 5e-324, 1e300]
            col = Array.from_numpy(t, v, valid)
        elif name == "i":
            col = Array.from_numpy(t, np.arange(n, dtype=np.int64))
        elif t == U8:
            idx = rng.integers(0, len(STRINGS), n)
            if n >= len(STRINGS):
                idx[:len(STRINGS)] = rng.permutation(len(STRINGS))
            col = Str([STRINGS[j] for j in idx], valid)
        elif t == BOOL:
            col = Array.from_numpy(t, rng.random(n) < 0.5, valid)
        elif t in FLOATS:
            col = Array.from_numpy(t, float_column(rng, t, n), valid)
        else:
            col = Array.from_numpy(t, int_column(rng, t, n), None if valid.all() else valid)
        cols.append(col)
    _tables[(n, seed)] = Table(FIELDS, cols)
    return _tables[(n, seed)]


def split_table(tab, sizes):
    out, lo = [], 0
    for sz in sizes:
        cols = []
        for c in tab.cols:
            if isinstance(c, Str):
                cols.append(Str(c.strings[lo:lo + sz], c.valid[lo:lo + sz]))
            else:
                m = c.valid_mask()[lo:lo + sz]
                cols.append(Array.from_numpy(c.data_type, np.array(c.numpy_values())[lo:lo + sz], None if m.all() else m))
        out.append(Table(tab.fields, cols))
        lo += sz
    return out


# -------------------------------------------------------------- the generator
LIT_SLOTS, STR_SLOTS, STR_BYTES, MAX_OUTPUTS = 32, 8, 256, 16  # jit_expr.cpp: Gen::lit, Gen::strlit; dfmi.h: 16 outputs


class Gen:
    """One query's generator state: the random source and what is left of the program limits."""

    def __init__(self, seed, utf8=True, boolcol=True):
        self.utf8 = utf8  # False: no Utf8 column anywhere (the numeric sub-tile form takes no Utf8 column)
        self.boolcol = boolcol  # False: no Boolean column either (the aggregate sub-tile form takes none)
        self.rng = random.Random(seed)
        self.lits, self.strs, self.str_bytes = LIT_SLOTS, STR_SLOTS, STR_BYTES

    # ---- leaves
    def literal(self, t=None):
        rng = self.rng
        if self.lits < 1:
            return None
        self.lits -= 1
        if t is None:
            t = rng.choice([I64, I64, F64])
        if t in FLOATS:
            return Literal(ScalarValue(t, rng.choice([0.5, -2.25, 0.0, 3.0, 1e6, -7.5])))
        return Literal(ScalarValue(t, rng.choice([0, 1, -1, 2, 3, 10, 100, -100, 127] if t != U64 else [0, 1, 2, 3, 10, 100])))

    def num_leaf(self):
        if self.rng.random() < 0.75:
            return Column(self.rng.choice(NUM_COLS))
        return self.literal() or Column(self.rng.choice(NUM_COLS))

    def string_literal(self):
        pool = [s for s in STR_LITERALS if len(s) <= self.str_bytes]
        if self.strs < 1 or not pool:
            return None
        s = self.rng.choice(pool)
        self.strs -= 1
        self.str_bytes -= len(s)
        return str_lit(s)

    # ---- coercion as the planner's
    def coerce(self, l, op, r):
        try:
            e = binary_expr_coerced(l, op, r, SCHEMA)
            return BinaryExpr(fold(e.left), op, fold(e.right))
        except PlanError:  # no common type the planner converts to (UInt64 against a signed type): both to Float64
            return BinaryExpr(to_f64(l), op, to_f64(r))

    def divisor(self, left_type, depth, literal_only=False, no_literal=False):
        """A divisor that is never zero and never -1: a literal, a dedicated
        column, or (Float64) abs(tree) + 1."""
        rng = self.rng
        k = rng.random()
        if literal_only or (k < 0.4 and not no_literal):
            if self.lits >= 2:
                self.lits -= 2  # (a literal Modulus divisor takes a second slot for its reciprocal)
                if left_type in FLOATS:
                    return Literal(ScalarValue(left_type, rng.choice([2.5, -3.0, 0.125, 7.0, 1e10])))
                vals = [2, 3, 7, 10, 16, 100] + ([-3, -7, -128] if left_type in SIGNED else [])
                return Literal(ScalarValue(left_type, rng.choice(vals)))
            if literal_only:
                return None
        if left_type in FLOATS and depth > 1 and k > 0.8 and self.lits >= 1:
            self.lits -= 1
            return BinaryExpr(fn("abs", to_f64(self.num(depth - 2, "fn"))), Operator.Plus, Literal(Float64(1.0)))
        return Column(DX if left_type in FLOATS else (D8 if left_type == I8 else DI))

    # ---- numeric trees
    NUM_KINDS = ["arith"] * 4 + ["divide"] * 2 + ["mod_lit"] * 3 + ["mod_col"] * 3 + ["cast_num"] * 2 + \
        ["cast_utf8_int"] * 2 + ["cast_utf8_float"] * 2 + ["cast_bool_num"] * 3 + ["fn"] * 8 + ["fn_mod"]
    NUM_EXT = {"modulus": ["mod_lit", "mod_col"], "fn": ["fn"] * 6 + ["fn_mod"],
               "cast_any": ["cast_utf8_int", "cast_utf8_float", "cast_bool_num"]}

    def num(self, depth, cross=None):
        """A numeric tree; `cross` names the parent's family: the child is then
        mostly taken from another family."""
        rng = self.rng
        if depth <= 0:
            return self.num_leaf()
        if cross is not None and rng.random() < 0.85:
            kind = rng.choice([k for fam, ks in self.NUM_EXT.items() if fam != cross for k in ks])
        elif rng.random() < 0.15:
            return self.num_leaf()
        else:
            kind = rng.choice(self.NUM_KINDS)
        if not self.utf8 and kind.startswith("cast_utf8"):
            kind = "cast_bool_num"
        d = depth - 1
        if kind == "arith":
            return self.coerce(self.num(d), rng.choice(MATH[:3]), self.num(d))
        if kind in ("divide", "mod_col"):
            l = self.num(d, "modulus" if kind == "mod_col" else None)
            op = Operator.Divide if kind == "divide" else Operator.Modulus
            return self.coerce(l, op, self.divisor(l.get_type(SCHEMA), d, no_literal=kind == "mod_col"))
        if kind == "mod_lit":
            l = self.num(d, "modulus")
            r = self.divisor(l.get_type(SCHEMA), d, literal_only=True)
            return BinaryExpr(l, Operator.Modulus, r) if r is not None else l
        if kind == "cast_num":
            x = self.num(d)
            if is_literal(x):
                return x
            return Cast(x, rng.choice([t for t in (I64, I32, I8, U64, F64, F32, T.Int16, T.UInt8) if t != x.get_type(SCHEMA)]))
        if kind == "cast_utf8_int":
            return Cast(Column(rng.choice([S, U])), rng.choice([I64, I64, I32, I8, U64, T.UInt16]))
        if kind == "cast_utf8_float":
            return Cast(Column(rng.choice([S, U])), rng.choice([F64, F64, F32]))
        if kind == "cast_bool_num":
            return Cast(self.boolean(d, "cast_any"), rng.choice([I64, I32, I8, U64, F64, F32]))
        if kind == "fn":
            return fn(rng.choice(UNARY), to_f64(self.num(d, "fn")))
        assert kind == "fn_mod"
        return fn("mod", to_f64(self.num(d, "fn")), to_f64(self.num(d, "fn")))

    # ---- Boolean trees
    BOOL_KINDS = ["cmp"] * 5 + ["andor"] * 4 + ["cast_utf8_bool"] * 2 + ["cast_num_bool"] * 7 + ["isnull"] * 3 + \
        ["utf8_eq"] * 2 + ["ord_lit"] * 3 + ["ord_col"] * 2 + ["column"]

    def bool_leaf(self):
        if self.boolcol:
            return Column(F)
        return self.coerce(Column(self.rng.choice(NUM_COLS)), self.rng.choice(CMP), self.num_leaf())

    def boolean(self, depth, cross=None):
        rng = self.rng
        if depth <= 0:
            return self.bool_leaf()
        if cross == "cast_any" and rng.random() < 0.6:
            kind = rng.choice(["ord_lit", "ord_lit", "ord_col"])
        else:
            kind = rng.choice(self.BOOL_KINDS)
        if not self.utf8 and kind in ("cast_utf8_bool", "utf8_eq", "ord_lit", "ord_col"):
            kind = "cast_num_bool"
        d = depth - 1
        if kind == "column":
            return self.bool_leaf()
        if kind == "cmp":
            return self.coerce(self.num(d), rng.choice(CMP), self.num(d))
        if kind == "andor":
            return BinaryExpr(self.boolean(d), rng.choice([Operator.And, Operator.Or]), self.boolean(d))
        if kind == "cast_utf8_bool":
            return Cast(Column(rng.choice([S, U])), BOOL)
        if kind == "cast_num_bool":
            x = self.num(d, "cast_any")
            return Cast(Column(self.rng.choice(NUM_COLS)) if is_literal(x) else x, BOOL)  # (no CAST of a literal to Boolean)
        if kind == "isnull":
            k = rng.random()
            x = Column(rng.choice([S, U])) if k < 0.2 and self.utf8 else (self.boolean(d) if k < 0.4 else self.num(d, "base"))
            return rng.choice([IsNull, IsNotNull])(x)
        if kind == "ord_col":
            l, r = rng.choice([(S, U), (U, S), (S, S)])
            return BinaryExpr(Column(l), rng.choice(ORDER_OPS), Column(r))
        op = rng.choice(ORDER_OPS) if kind == "ord_lit" else rng.choice([Operator.Eq, Operator.NotEq])
        if kind == "utf8_eq" and rng.random() < 0.3:
            return BinaryExpr(Column(S), op, Column(U))
        q = self.string_literal()
        if q is None:
            return BinaryExpr(Column(S), op, Column(U))
        c = Column(rng.choice([S, U]))
        return BinaryExpr(q, op, c) if rng.random() < 0.5 else BinaryExpr(c, op, q)


def fn(name, *args):
    return ScalarFunction(name, tuple(args), F64)


def fold(e):
    """A cast of a literal is compiled only from Int64 to Float64 (expression.rs:
    291-305): any other becomes the literal of the target type."""
    if isinstance(e, Cast) and isinstance(e.expr, Literal) and (e.expr.value.dtype, e.data_type) != (I64, F64):
        v = e.expr.value.value
        return Literal(ScalarValue(e.data_type, float(v) if e.data_type in FLOATS else int(v)))
    return e


def to_f64(e):
    return fold(e.cast_to(F64, SCHEMA))


def gen_query(seed, predicate=None, utf8=True):
    """(pred or None, 1-4 projections): about one query in four has no
    predicate (`predicate` forces one or none)."""
    g = Gen(seed, utf8)
    rng = g.rng
    has_pred = rng.random() >= 0.25 if predicate is None else predicate
    depth = lambda: rng.choice([1, 2, 3, 3, 4, 4])
    pred = g.boolean(depth()) if has_pred else None
    projs = []
    for _ in range(rng.randrange(1, 5)):
        k = rng.random()
        if k < 0.1:
            projs.append(Column(rng.choice([S, U, A, F, Y] if utf8 else [A, F, Y])))  # passed through
        elif k < 0.3:
            projs.append(g.boolean(depth()))
        else:
            projs.append(g.num(depth()))
    assert len(projs) <= MAX_OUTPUTS
    return pred, projs


def gen_numeric_tree(seed, depth=3, subtile=False):
    """(pred or None, one numeric tree): an aggregate's argument. `subtile`:
    always a predicate, and neither a Utf8 nor a Boolean column anywhere, so
    that the aggregate kernel's sub-tile form takes the query."""
    g = Gen(seed, utf8=not subtile, boolcol=not subtile)
    pred = g.boolean(g.rng.randrange(1, 4)) if g.rng.random() >= 0.25 or subtile else None
    return pred, g.num(depth, g.rng.choice([None, "fn", "modulus", "cast_any"]))


def aggregates_of(e):
    """SUM / MIN / MAX / COUNT of one numeric tree."""
    t = e.get_type(SCHEMA)
    return [AggregateFunction("SUM", (e,), t), AggregateFunction("MIN", (e,), t), AggregateFunction("MAX", (e,), t),
            AggregateFunction("COUNT", (e,), T.UInt64)]


def gen_group_key(seed, window):
    """A GROUP BY key: (CAST(abs(tree) AS BIGINT) % 1000 + i) % 16 -- a
    non-negative value reduced to 16 values and the null key, inside the fused
    key window -- or a Float64 tree of few distinct values, the hash table's
    fused pass."""
    g = Gen(seed)
    pred = g.boolean(g.rng.randrange(1, 4)) if g.rng.random() >= 0.5 else None
    lit = lambda v: Literal(Int64(v))
    if window:
        x = BinaryExpr(Cast(fn("abs", to_f64(g.num(2, "fn"))), I64), Operator.Modulus, lit(1000))
        key = BinaryExpr(BinaryExpr(x, Operator.Plus, Column(I)), Operator.Modulus, lit(16))
    else:
        x = fn(g.rng.choice(["floor", "round", "trunc"]),
               fn("mod", to_f64(g.num(2, "fn")), Literal(Float64(g.rng.choice([8.0, 12.5])))))
        key = BinaryExpr(x, Operator.Plus, fn("mod", Cast(Column(I), F64), Literal(Float64(4.0))))
    return pred, key


# the seeds of the GPU tests (tests/test_compose_cpu.py checks every one of them on the CPU)
SEEDS = list(range(26000, 26096))        # filter + project at ROWS rows: 16 cases of 6
SMALL_SEEDS = list(range(26096, 26102))  # ... at ROWS_SMALL rows
SUBTILE_SEEDS = list(range(27000, 27016))  # Utf8-free with a predicate: the numeric sub-tile form takes them
AGG_SEEDS = list(range(28000, 28012))
AGG_SUBTILE_SEEDS = list(range(28100, 28112))  # gen_numeric_tree(subtile=True): the aggregate sub-tile form takes them
GROUP_SEEDS = list(range(29000, 29008))  # even: the key window; odd: the hash table
ORDER_SEEDS = list(range(30000, 30008))


def subtile_query(seed):
    return gen_query(seed, predicate=True, utf8=False)


def takes_subtile_form(pred, projs):
    """The numeric sub-tile kernel takes a query with a predicate over at
    least one column and no Utf8 column anywhere (exec_plan.cpp)."""
    if pred is None:
        return False
    cols = [e for tree in [pred] + list(projs) for e in postfix(tree) if isinstance(e, Column)]
    return all(e.get_type(SCHEMA) != U8 for e in cols) and any(isinstance(e, Column) for e in postfix(pred))


def literal_chain(n=17):
    """(a > 0, x + 1.0 + 2.0 + ... + n.0): the smallest tree that a kernel form
    emitting its argument twice with new literal slots each time refused --
    more than 16 literals, 32 being the limit."""
    e = Column(X)
    for k in range(1, n + 1):
        e = BinaryExpr(e, Operator.Plus, Literal(Float64(float(k))))
    return BinaryExpr(Column(A), Operator.Gt, Literal(Int64(0))), e


def takes_agg_subtile_form(pred, tree):
    """The aggregate kernel's sub-tile form takes an ungrouped query with a
    predicate that reads no Utf8 and no Boolean column (aggregate.cpp)."""
    if pred is None:
        return False
    cols = [e for t in (pred, tree) for e in postfix(t) if isinstance(e, Column)]
    return all(e.get_type(SCHEMA) not in (U8, BOOL) for e in cols)


def order_key(seed):
    return Gen(seed).num(3, "base")


# ---------------------------------------------------------------- node kinds
# Two limits of the (parent kind, child kind) matrix below. CAST from Utf8 and
# the Boolean <-> numeric casts count as one family (they came under one flag,
# DFMI_FLAG_EXT_CAST_ANY), so a pair inside it, such as CAST(CAST(s AS INT) AS
# BOOLEAN), is generated by chance and not required. And a pair does not say
# which operand the child is: a generated Modulus or Divide takes an
# extension node as its dividend only -- its divisor is a literal, a
# dedicated column (under the planner's cast) or abs(tree) + 1, so that no
# value query raises -- and a parsed string as a divisor runs only in the
# error templates.
FAMILY = {"mod_lit": "modulus", "mod_col": "modulus", "fn_mod": "fn", "cast_utf8_int": "cast_any",
          "cast_utf8_float": "cast_any", "cast_utf8_bool": "cast_any", "cast_bool_num": "cast_any",
          "cast_num_bool": "cast_any", "ord_lit": "order", "ord_col": "order"}
FAMILY.update({"fn_" + nm: "fn" for nm in UNARY})
BASE_KINDS = ["column", "literal", "arith", "divide", "cmp", "andor", "cast_num", "isnull", "utf8_eq"]
KINDS = BASE_KINDS + list(FAMILY)


def is_literal(e):
    return isinstance(e, Literal) or (isinstance(e, Cast) and isinstance(e.expr, Literal))  # (the planner's folded cast)


def kind_of(e):
    if isinstance(e, Column):
        return "column"
    if isinstance(e, Literal):
        return "literal"
    if isinstance(e, (IsNull, IsNotNull)):
        return "isnull"
    if isinstance(e, ScalarFunction):
        return "fn_" + e.name
    if isinstance(e, Cast):
        src = e.expr.get_type(SCHEMA)
        if src == U8:
            return "cast_utf8_bool" if e.data_type == BOOL else ("cast_utf8_float" if e.data_type in FLOATS else "cast_utf8_int")
        if src == BOOL:
            return "cast_bool_num"
        return "cast_num_bool" if e.data_type == BOOL else "cast_num"
    if e.op in (Operator.And, Operator.Or):
        return "andor"
    if e.op == Operator.Modulus:
        return "mod_lit" if is_literal(e.right) else "mod_col"
    if e.op in MATH:
        return "divide" if e.op == Operator.Divide else "arith"
    if not is_utf8_operand(e.left, EMPTY):
        return "cmp"
    if e.op in ORDER_OPS:
        return "ord_col" if isinstance(e.left, Column) and isinstance(e.right, Column) else "ord_lit"
    return "utf8_eq"


def children(e):
    if isinstance(e, BinaryExpr):
        return [e.left, e.right]
    if isinstance(e, ScalarFunction):
        return list(e.args)
    if isinstance(e, (Cast, IsNull, IsNotNull)):
        return [e.expr]
    return []


def kinds_and_pairs(e, kinds, pairs):
    """Counts e's node kinds into `kinds` and its (parent kind, child kind)
    pairs into `pairs`; a numeric coercion cast between the two is looked through."""
    k = kind_of(e)
    kinds[k] = kinds.get(k, 0) + 1
    for c in children(e):
        kinds_and_pairs(c, kinds, pairs)
        while kind_of(c) == "cast_num":
            c = c.expr
        pairs.add((k, kind_of(c)))


# ------------------------------------------------------------ error templates
ERR_COLS = [("a", I64, True), ("b", I64, False), ("c", I64, False), ("d", I64, False), ("s", U8, True), ("x", F64, False),
            ("w", F64, False)]
EA, EB, EC, ED, ES, EX, EW = range(len(ERR_COLS))
ERR_FIELDS = [Field(n, t, nullable) for n, t, nullable in ERR_COLS]
MIN64 = np.iinfo(np.int64).min


def error_table(edits, null_a=(), null_s=(), n=ROWS):
    """a = 100.., b = 7, c = 50.., d = 3, s = a number's rendering, x in [1, 2),
    w = the row index; `edits` = [(column, row, value)]."""
    rng = np.random.default_rng(3)
    vals = {EA: np.arange(n, dtype=np.int64) % 90 + 100, EB: np.full(n, 7, np.int64), EC: np.arange(n, dtype=np.int64) % 40 + 50,
            ED: np.full(n, 3, np.int64), ES: [repr(float(v)).encode() for v in rng.random(n) * 100], EX: rng.random(n) + 1,
            EW: np.arange(n, dtype=np.float64)}
    for c, r, v in edits:
        vals[c][r] = v
    va, vs = np.ones(n, bool), np.ones(n, bool)
    va[list(null_a)] = False
    vs[list(null_s)] = False
    cols = [Array.from_numpy(I64, vals[EA], None if va.all() else va), Array.from_numpy(I64, vals[EB]),
            Array.from_numpy(I64, vals[EC]), Array.from_numpy(I64, vals[ED]), Str(vals[ES], vs), Array.from_numpy(F64, vals[EX]),
            Array.from_numpy(F64, vals[EW])]
    return Table(ERR_FIELDS, cols)


def error_cases():
    """[(name, table, pred, projs, the planted error or None)]: a Divide D, a
    Modulus M and a Utf8 -> Float64 cast P at the digit limit, composed with
    the function and Boolean-cast families; the planted rows are in both tiles."""
    col = Column
    D = BinaryExpr(col(EA), Operator.Divide, col(EB))
    M = BinaryExpr(col(EC), Operator.Modulus, col(ED))
    P = Cast(col(ES), F64)
    f64 = lambda e: Cast(e, F64)
    plus = lambda l, r: BinaryExpr(l, Operator.Plus, r)
    dmp = plus(plus(f64(D), fn("sqrt", fn("abs", f64(M)))), fn("floor", P))  # ordinals: D, then M, then P
    pmd = plus(plus(fn("floor", P), fn("sqrt", fn("abs", f64(M)))), f64(D))  # ... P, then M, then D
    lim = lambda r: (ES, r, LIMIT_STRING)
    lt = lambda e, v: BinaryExpr(e, Operator.Lt, Literal(Float64(v)))
    cases = [
        # one projection: the lowest ordinal wins whatever the rows are
        ("one_projection_divide_first", error_table([(EB, 4100, 0), (EC, 10, MIN64), (ED, 10, -1), lim(5)]), None, [dmp], DIV0),
        ("one_projection_modulus_before_cast", error_table([(EC, 4000, MIN64), (ED, 4000, -1), lim(5)]), None, [dmp],
         REM_OVERFLOW),
        ("one_projection_cast_first", error_table([(EB, 3, 0), (ED, 10, 0), lim(4101)]), None, [pmd], limit_error(F64)),
        # two projections: the first projection's nodes come first
        ("two_projections_modulus_in_the_first", error_table([(ED, 4000, 0), (EA, 1, MIN64), (EB, 1, -1)]), None,
         [fn("sqrt", fn("abs", f64(M))), BinaryExpr(f64(D), Operator.Multiply, P)], DIV0),
        ("two_projections_cast_before_divide_in_the_second", error_table([lim(2000), (EA, 1, MIN64), (EB, 1, -1)]), None,
         [fn("round", f64(M)), plus(fn("floor", P), f64(D))], limit_error(F64)),
        # the predicate's nodes come before every projection's
        ("predicate_modulus_before_projection_divide", error_table([(EC, 4104, MIN64), (ED, 4104, -1), (EB, 0, 0)]),
         BinaryExpr(Cast(BinaryExpr(M, Operator.Eq, Literal(Int64(1))), I64), Operator.GtEq, Literal(Int64(0))), [D],
         REM_OVERFLOW),
        ("projection_divide_after_a_clean_predicate_cast_and_a_clean_modulus", error_table([(EA, 4099, MIN64), (EB, 4099, -1)]),
         lt(fn("floor", P), 1000.0), [M, D], DIV_OVERFLOW),
        # a failing row the predicate deselects raises nothing: the later node's selected row does
        ("deselected_failing_row", error_table([(ED, 20, 0), (EW, 20, 1e9), (EA, 4098, MIN64), (EB, 4098, -1)]),
         lt(col(EW), 1e6), [fn("ceil", f64(M)), D], DIV_OVERFLOW),
        # b = 0 where a is null: no error at the Divide; the Modulus after it fails
        ("failing_row_whose_other_operand_is_null", error_table([(EB, 5, 0), (EC, 900, MIN64), (ED, 900, -1)], null_a=[5]),
         None, [dmp], REM_OVERFLOW),
        # c % CAST(s AS BIGINT): an unparseable string and a null row are null divisors with zero slots
        ("zero_divisor_that_is_an_unparseable_strings_null",
         error_table([(ES, 7, b"x"), (ES, 4100, b"0"), (ES, 8, b"1.5")] + [(ES, r, b"%d" % (r % 9 + 2)) for r in range(9, ROWS)
                                                                             if r != 4100],
                     null_s=[4100]),
         None, [BinaryExpr(col(EC), Operator.Modulus, Cast(col(ES), I64)),
                fn("sqrt", f64(BinaryExpr(col(EC), Operator.Modulus, Cast(col(ES), I64))))], None),
        # a mixed-type math node's static error against a device error
        ("static_error_after_a_device_error", error_table([(EB, 4100, 0)]), None, [D, plus(col(EA), col(EX))], DIV0),
        ("static_error_before_a_device_error", error_table([(EB, 0, 0)]), None,
         [plus(BinaryExpr(col(EC), Operator.Modulus, Literal(Int64(7))), col(EX)), D], MATH_OPS),
    ]
    return cases
