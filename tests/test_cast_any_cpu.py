"""CAST from Utf8 and Boolean (DFMI_FLAG_EXT_CAST_ANY), the parts that need no
GPU: the unchanged compile errors without both flags, names / types with them,
the ABI surface, the generated kernels compiled for gfx950, planning and the
wire format, a Python restatement of the contract pinned on a corpus and on
the native CSV reader, and the parsers -- the skeleton's own text -- under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/native/cast_parse_driver.cpp).

The restatement (`restate`) is what tests/test_gpu_cast_any.py compares the
device with: the oracle executes no CAST of a column."""
import os
import re
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from datafusion_amd import _abi, serde
from datafusion_amd.arrow import Field, Schema
from datafusion_amd.execution import ExecutionContext, MemoryDataSource
from datafusion_amd.execution.datasource import NativeCsvDataSource
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.execution.expression import compile_scalar_expr
from datafusion_amd.logicalplan import (AggregateFunction, BinaryExpr, Cast, Column, DataType, Float64, Int64, Literal,
                                        Operator, ScalarValue, Utf8)
from datafusion_amd.sqlplanner import SqlToRel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAST = _abi.DFMI_FLAG_EXT_CAST
ANY = getattr(_abi, "DFMI_FLAG_EXT_CAST_ANY", 0x800)
BOTH = CAST | ANY
U8C = _abi.DFMI_FLAG_EXT_UTF8_COMPARE

INTS = [DataType.Int8, DataType.Int16, DataType.Int32, DataType.Int64,
        DataType.UInt8, DataType.UInt16, DataType.UInt32, DataType.UInt64]
FLOATS = [DataType.Float32, DataType.Float64]
NUMERIC = INTS + FLOATS
TARGETS = [DataType.Boolean] + NUMERIC
LIMIT = "limit"  # what restate returns for a row that raises the program limit


def limit_message(t):
    return "device program limit: CAST to %s needs more than 19 significant digits" % t.name


# ------------------------------------------------------------ the restatement
INT_RE = re.compile(rb"([+-]?)([0-9]+)\Z")
FLOAT_RE = re.compile(rb"([+-]?)(?:(inf|infinity|nan)|(?:([0-9]*)(\.?)([0-9]*))(?:[eE]([+-]?[0-9]+))?)\Z", re.I)
FMT = {DataType.Float64: (53, -1022, 1023), DataType.Float32: (24, -126, 127)}


def round_to(v, t):
    """The non-negative Fraction v rounded to the float type t, nearest, ties
    to even, subnormals at their quantum, inf past the range: its bits."""
    p, emin, emax = FMT[t]
    inf = ((1 << (8 * t.width - p)) - 1) << (p - 1)
    if v == 0:
        return 0
    e = v.numerator.bit_length() - v.denominator.bit_length()  # 2^(e-1) <= v < 2^(e+1)
    if v < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    q = max(e, emin) - (p - 1)  # the quantum's exponent
    n = v / Fraction(2) ** q
    r = n.numerator // n.denominator
    rem = n - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (r & 1)):
        r += 1
    if r == 0:
        return 0
    if r < (1 << (p - 1)):
        return r  # subnormal
    if r == (1 << p):
        r >>= 1
        q += 1
    ex = q + p - 1
    if ex > emax:
        return inf
    return ((ex - emin + 1) << (p - 1)) | (r - (1 << (p - 1)))


def restate(s, t):
    """CAST(s AS t) of the byte string s: None for a null, LIMIT for the
    program limit, else the value -- a bool, an int, or the float's bits."""
    if t == DataType.Boolean:
        low = s.lower() if all(c < 0x80 for c in s) else b""
        return True if low == b"true" else (False if low == b"false" else None)
    if t in INTS:
        m = INT_RE.match(s)
        signed = t in INTS[:4]
        if not m or (m.group(1) == b"-" and not signed):
            return None
        v = int(m.group(2)) * (-1 if m.group(1) == b"-" else 1)
        bits = 8 * t.width
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        return v if lo <= v <= hi else None
    m = FLOAT_RE.match(s)
    if not m:
        return None
    p, emin, emax = FMT[t]
    top = 8 * t.width - 1
    sign = (1 << top) if m.group(1) == b"-" else 0
    inf = ((1 << (top + 1 - p)) - 1) << (p - 1)
    if m.group(2):
        return sign | (inf if m.group(2).lower() != b"nan" else inf | (1 << (p - 2)))
    ip, fp = m.group(3), m.group(5)
    if not ip and not fp:
        return None
    digits = (ip + fp).lstrip(b"0")
    if not digits:
        return sign
    ex = int(m.group(6) or b"0") - len(fp)  # the value is digits * 10^ex
    if ex + len(digits) > 400:
        return sign | inf
    if ex + len(digits) < -400:
        return sign
    ten = lambda k: Fraction(10) ** k
    if len(digits) > 19 and digits[19:].strip(b"0"):
        w, e = int(digits[:19]), ex + len(digits) - 19
        lo, hi = round_to(w * ten(e), t), round_to((w + 1) * ten(e), t)
        if lo != hi:
            return LIMIT
        assert round_to(int(digits) * ten(ex), t) == lo
        return sign | lo
    return sign | round_to(int(digits) * ten(ex), t)


def float_bits(x, t):
    return struct.unpack("<Q", struct.pack("<d", x))[0] if t == DataType.Float64 else \
        struct.unpack("<I", struct.pack("<f", x))[0]


# ----------------------------------------------------------------- the corpus
def int_edges():
    out = []
    for bits in (8, 16, 32, 64):
        for v in (-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -(1 << (bits - 1)) - 1, 1 << (bits - 1),
                  (1 << bits) - 1, 1 << bits, -1):
            out.append(str(v).encode())
    return out


CORPUS = [b"", b"+", b"-", b"0", b"-0", b"+0", b"007", b"0" * 100 + b"1"] + int_edges() + [
    b"-1", b"+5", b" 5", b"5 ", b"5.0", b"1e3", b"1_0", "٣".encode(), b"1\x002",
    str((1 << 64) - 1).encode(), str(1 << 64).encode(), str((1 << 64) + 1).encode(), b"1234567890" * 4,
    b"true", b"TRUE", b"False", b"t", b"1",
    b"1.", b".5", b".", b"+.5e-3", b"1e", b"1e+", b"e5", b"1e5.0", b"0x10",
    b"inf", b"-Infinity", b"+NaN", b"-nan", b"infinit",
    b"1e400", b"-1e-400", b"4.9e-324", b"2.4703282292062327e-324", b"2.4703282292062328e-324",
    b"1.7976931348623158e308", b"1.7976931348623159e308", b"9007199254740993", b"16777217.0000000001",
    b"0." + b"0" * 400 + b"1", b"1" + b"0" * 30, b"1e0000000000000000005", b"1e99999999999999999999", b"0e99999999999",
    b"9007199254740992.9999999999999999999", b"9007199254740993.0000000000000000001",
]
LIMIT_STRING = b"9007199254740993.0000000000000000001"

# (string, Float64 bits, Float32 bits); None: a null
F64_KNOWN = {
    b"1": 0x3FF0000000000000, b"1.": 0x3FF0000000000000, b".5": 0x3FE0000000000000, b".": None,
    b"+.5e-3": float_bits(0.0005, DataType.Float64), b"1e": None, b"1e+": None, b"e5": None, b"1e5.0": None, b"0x10": None,
    b"inf": 0x7FF0000000000000, b"-Infinity": 0xFFF0000000000000, b"+NaN": 0x7FF8000000000000, b"-nan": 0xFFF8000000000000,
    b"infinit": None, b"1e400": 0x7FF0000000000000, b"-1e-400": 0x8000000000000000, b"4.9e-324": 1,
    b"2.4703282292062327e-324": 0, b"2.4703282292062328e-324": 1, b"1.7976931348623158e308": 0x7FEFFFFFFFFFFFFF,
    b"1.7976931348623159e308": 0x7FF0000000000000, b"9007199254740993": 0x4340000000000000,
    b"0." + b"0" * 400 + b"1": 0, b"1" + b"0" * 30: float_bits(1e30, DataType.Float64),
    b"1e0000000000000000005": float_bits(1e5, DataType.Float64), b"1e99999999999999999999": 0x7FF0000000000000,
    b"0e99999999999": 0, b"9007199254740992.9999999999999999999": 0x4340000000000000, LIMIT_STRING: LIMIT,
    b"": None, b"+": None, b"-0": 0x8000000000000000, b" 5": None, b"5 ": None, b"1_0": None, b"true": None,
}
F32_KNOWN = {b"16777217.0000000001": float_bits(16777218.0, DataType.Float32), b"-nan": 0xFFC00000, b"+NaN": 0x7FC00000,
             b"1e400": 0x7F800000, b"-1e-400": 0x80000000, b"4.9e-324": 0, b"1e-45": 1, b"7e-46": 0, b"7.1e-46": 1,
             b"3.4028235e38": 0x7F7FFFFF, b"3.4028236e38": 0x7F800000, LIMIT_STRING: float_bits(2.0 ** 53, DataType.Float32)}


def test_restatement_on_the_corpus():
    for s, want in F64_KNOWN.items():
        assert restate(s, DataType.Float64) == want, s
    for s, want in F32_KNOWN.items():
        assert restate(s, DataType.Float32) == want, s
    for s in CORPUS:
        if restate(s, DataType.Float64) not in (None, LIMIT) and b"nan" not in s.lower():
            # CPython's float() is correctly rounded too (it also takes blanks and '_', which FLOAT_RE rejects)
            assert restate(s, DataType.Float64) == float_bits(float(s.decode()), DataType.Float64), s
    i64 = lambda s: restate(s, DataType.Int64)
    assert [i64(s) for s in (b"", b"+", b"-", b"0", b"-0", b"+0", b"007", b"0" * 100 + b"1")] == [None, None, None, 0, 0, 0, 7, 1]
    assert [i64(s) for s in (b" 5", b"5 ", b"5.0", b"1e3", b"1_0", "٣".encode(), b"1\x002", b"+5")] == [None] * 7 + [5]
    assert restate(b"-0", DataType.UInt8) is None and restate(b"+0", DataType.UInt8) == 0
    for t in INTS:
        bits, signed = 8 * t.width, t in INTS[:4]
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        assert [restate(str(v).encode(), t) for v in (lo, hi, lo - 1, hi + 1)] == [lo, hi, None, None], t
    assert [restate(s, DataType.Boolean) for s in (b"true", b"TRUE", b"False", b"t", b"1", b"")] == \
        [True, True, False, None, None, None]
    assert restate(LIMIT_STRING, DataType.Int64) is None


def random_strings(n, seed, long_too=False):
    """Strings of at most 19 significant digits (integers of 1 to 19 digits,
    repr of random doubles, shortest Float32 renderings) and a few that do not parse."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        k = i % 8
        if k < 3:
            v = int(rng.integers(0, 10 ** int(rng.integers(1, 19))))
            out.append(("-" if k == 1 else "") + str(v))
        elif k == 3:
            out.append(repr(float(np.frombuffer(rng.bytes(8), np.float64)[0])).replace("nan", "1.5").replace("inf", "2.5"))
        elif k == 4:
            out.append(repr(float(rng.standard_normal() * 10.0 ** int(rng.integers(-20, 20)))))
        elif k == 5:
            out.append(str(np.float32(rng.standard_normal() * 1000)))
        elif k == 6:
            out.append("%d.%0*d" % (int(rng.integers(0, 1000)), int(rng.integers(1, 9)), int(rng.integers(0, 10 ** 8)))
                       if long_too else str(int(rng.integers(-200, 200))))
        else:
            out.append(["x", "1 ", "--1", "1e", "true", "FALSE", "12a", "0.5.1", "NaN", "-inf"][int(rng.integers(0, 10))])
    return [s.encode() for s in out]


@pytest.mark.parametrize("t", TARGETS, ids=[t.name for t in TARGETS])
def test_restatement_against_the_csv_reader(t, tmp_path):
    """One generated one-column file: every field the restatement gives a value
    for reads back with those bits; every other string (but the empty one,
    the reader's null) alone in a file is the reader's parse error. (`-nan`: the reader
    drops the sign of a NaN, Rust's parse and this contract keep it -- compared
    without the sign.)"""
    strings = [s for s in CORPUS + random_strings(400, 5) if b"\n" not in s and b"," not in s and b'"' not in s]
    strings = [s for s in strings if restate(s, t) is not LIMIT]
    good = [s for s in strings if restate(s, t) is not None]  # (the empty field is the reader's null, no parse)
    bad = [s for s in strings if restate(s, t) is None and s != b""]
    assert len(good) > 10 and len(bad) > 20
    schema = Schema([Field("c", t, True)])
    path = tmp_path / "good.csv"
    path.write_bytes(b"".join(s + b"\n" for s in good))
    rb = NativeCsvDataSource(schema, str(path), has_header=False, batch_size=1 << 16).next()
    col = rb.columns[0]
    assert col.length == len(good)
    valid, vals = col.valid_mask(), np.array(col.numpy_values())
    for i, s in enumerate(good):
        want = restate(s, t)
        assert bool(valid[i]) == (want is not None), s
        if want is None:
            continue
        if t in FLOATS:
            got = int(vals[i:i + 1].view("u%d" % t.width)[0])
            if s.lower() == b"-nan":
                want &= ~(1 << (8 * t.width - 1))
            assert got == want, (s, hex(got), hex(want))
        else:
            assert vals[i] == want, (s, vals[i], want)
    for s in bad[:60]:
        one = tmp_path / "bad.csv"
        one.write_bytes(s + b"\n")
        with pytest.raises(ExecutionError):
            NativeCsvDataSource(schema, str(one), has_header=False, batch_size=16).next()


# ------------------------------------------------------------------ front end
S = Schema([Field("c_%s" % t.name.lower(), t, True) for t in NUMERIC] +
           [Field("s", DataType.Utf8, True), Field("f", DataType.Boolean, True)])
SCOL, BCOL = len(NUMERIC), len(NUMERIC) + 1


def compiled(e, flags):
    try:
        r = compile_scalar_expr(None, e, S, flags)
        return ("ok", r.get_name(), r.get_type())
    except ExecutionError as x:
        return ("err", x.kind, x.message)


def new_forms():
    out = [(Cast(Column(SCOL), t), "Utf8", t) for t in TARGETS]
    out += [(Cast(Column(BCOL), t), "Boolean", t) for t in NUMERIC]
    out += [(Cast(Column(i), DataType.Boolean), NUMERIC[i].name, DataType.Boolean) for i in range(len(NUMERIC))]
    out.append((Cast(BinaryExpr(Column(3), Operator.Gt, Literal(Int64(5))), DataType.Int32), "Boolean", DataType.Int32))
    return out


@pytest.mark.parametrize("flags", [0, CAST, ANY, CAST | U8C | 0x7F0, ANY | U8C | 0x7F0])
def test_without_both_flags_every_new_form_fails_as_before(flags):
    for e, frm, t in new_forms():
        if flags & CAST:
            want = ("err", "NotImplemented", "CAST from %s to %s" % (frm, t.name))
        elif isinstance(e.expr, Column):
            want = ("err", "ExecutionError", "column reference")
        else:
            want = ("err", "General", "CAST not implemented for expression %r" % (e.expr,))
        assert compiled(e, flags) == want, (e, flags)


def test_names_and_types_with_both_flags():
    for e, frm, t in new_forms():
        assert compiled(e, BOTH) == ("ok", repr(e), t), e
    assert compiled(Cast(Column(SCOL), DataType.Int64), BOTH)[1] == "CAST(#%d AS Int64)" % SCOL
    # a cast result is an operand like any other
    e = BinaryExpr(Cast(Column(SCOL), DataType.Float64), Operator.Lt, Literal(Float64(2.5)))
    assert compiled(e, BOTH) == ("ok", repr(e), DataType.Boolean)


def test_excluded_forms_keep_their_text():
    f = BOTH | U8C
    assert compiled(Cast(Column(3), DataType.Utf8), f) == ("err", "NotImplemented", "CAST from Int64 to Utf8")
    assert compiled(Cast(Column(BCOL), DataType.Utf8), f) == ("err", "NotImplemented", "CAST from Boolean to Utf8")
    assert compiled(Cast(Column(SCOL), DataType.Utf8), f) == ("err", "NotImplemented", "CAST from Utf8 to Utf8")
    assert compiled(Cast(Column(BCOL), DataType.Boolean), f) == ("err", "NotImplemented", "CAST from Boolean to Boolean")
    lit = Cast(Literal(Utf8("12")), DataType.Int64)
    assert compiled(lit, f) == compiled(lit, CAST | U8C) and compiled(lit, f)[:2] == ("err", "NotImplemented")
    # Boolean comparisons stay run-time comparison_ops errors: they compile as before
    e = BinaryExpr(Column(BCOL), Operator.Eq, Column(BCOL))
    assert compiled(e, f) == compiled(e, CAST | U8C)
    # numeric casts are what they were
    assert compiled(Cast(Column(3), DataType.Float64), BOTH) == compiled(Cast(Column(3), DataType.Float64), CAST)


def test_flag_is_declared_and_the_version_stays_4():
    hdr = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    m = re.search(r"#define\s+DFMI_FLAG_EXT_CAST_ANY\s+(0x[0-9a-fA-F]+)u", hdr)
    assert m and m.group(1) == "0x800" and _abi.DFMI_FLAG_EXT_CAST_ANY == 0x800
    assert "pub const DFMI_FLAG_EXT_CAST_ANY: u32 = 0x800;" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define DFMI_ABI_VERSION 4\b", hdr)
    assert _abi.DFMI_ABI_VERSION == 4 and _abi.lib().dfmi_abi_version() == 4
    skel = open(os.path.join(ROOT, "datafusion_amd", "csrc", "jit_skeleton.hip")).read()
    assert re.search(r"ERRK_CAST_DIGITS\s*=\s*6\b", skel)


# ------------------------------------------------------- generated kernels
def body_of(src):
    return src[src.rindex('extern "C" __global__'):]


CT = {"Boolean": "bool", "Float32": "float", "Float64": "double"}
ctype = lambda t: CT.get(t.name, t.name.lower().replace("uint", "u").replace("int", "i"))
US = Schema([Field("s", DataType.Utf8, True), Field("v", DataType.Int64, False), Field("b", DataType.Boolean, True),
             Field("x", DataType.Float64, True)])


def below(t):  # CAST(s AS t) < 100 (Boolean: the cast itself)
    c = Cast(Column(0), t)
    if t == DataType.Boolean:
        return c
    return BinaryExpr(c, Operator.Lt, Literal(ScalarValue(t, 100.0 if t in FLOATS else 100)))


def test_dense_projection_of_every_target_compiles():
    from test_jit_cpu import jit_check
    rc, code, msg, src = jit_check(US, None, [Cast(Column(0), t) for t in TARGETS], BOTH, compile_=True)
    assert rc > 0, msg
    body = body_of(src)
    for t in TARGETS:
        assert "dfmi::utf8_parse<%s>(A, 0, row, " % ctype(t) in body, t
    assert body.count("ERRK_CAST_DIGITS") == 2 and "ERRK_CAST_DIGITS_F32" in body


def test_boolean_casts_are_plain_expressions():
    from test_jit_cpu import jit_check
    projs = [Cast(Column(2), t) for t in NUMERIC] + [Cast(Column(3), DataType.Boolean), Cast(Column(1), DataType.Boolean),
                                                    Cast(BinaryExpr(Column(3), Operator.Gt, Literal(Float64(0.5))), DataType.Int64)]
    rc, code, msg, src = jit_check(US, None, projs, BOTH, compile_=True)
    assert rc > 0, msg
    body = body_of(src)
    assert "utf8_parse" not in body and "num_cast" not in body and "ERRK_CAST" not in body
    assert "!= (double)0" in body and "!= (i64)0" in body


def all_targets_predicate():
    pred = below(TARGETS[0])
    for t in TARGETS[1:]:
        pred = BinaryExpr(pred, Operator.And, below(t))
    return pred


@pytest.mark.parametrize("batched", [False, True], ids=["device", "coalesced"])
def test_predicate_of_every_target_compiles(batched):
    from test_jit_cpu import jit_check
    flags = BOTH | (0x40000000 if batched else 0)
    projs = [Column(1), Cast(Column(0), DataType.Int64), Cast(Column(0), DataType.Float32)]
    rc, code, msg, src = jit_check(US, all_targets_predicate(), projs, flags, compile_=True)
    assert rc > 0, msg
    body = body_of(src)
    for t in TARGETS:
        assert "dfmi::utf8_parse<%s>(A, 0, row, " % ctype(t) in body, t
    assert ("batch_ptrs" in body) == batched


def test_dense_projection_in_the_coalesced_form_compiles():
    from test_jit_cpu import jit_check
    rc, code, msg, src = jit_check(US, None, [Cast(Column(0), t) for t in TARGETS], BOTH | 0x40000000, compile_=True)
    assert rc > 0, msg
    assert "batch_ptrs" in body_of(src)


def test_aggregate_arguments_of_every_target_compile():
    from test_aggregate_cpu import _agg_jit
    flags = BOTH | _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_GATHER_ALL
    aggs = [AggregateFunction("SUM", (Cast(Column(0), t),), t) for t in NUMERIC]
    aggs += [AggregateFunction("COUNT", (Cast(Column(0), DataType.Boolean),), DataType.UInt64),
             AggregateFunction("SUM", (Cast(Column(2), DataType.Int32),), DataType.Int32),
             AggregateFunction("SUM", (Cast(BinaryExpr(Column(3), Operator.Gt, Literal(Float64(0.5))), DataType.Int64),),
                               DataType.Int64)]
    for pred in (None, below(DataType.Float64)):
        rc, code, msg, src = _agg_jit(US, pred, aggs, flags)
        assert rc > 0, msg
        body = body_of(src)
        for t in TARGETS:
            assert "dfmi::utf8_parse<%s>(A, 0, row, " % ctype(t) in body, t


def test_grouped_kernel_with_a_parsed_key_compiles():
    from test_aggregate_cpu import _grouped_jit
    flags = BOTH | _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_GATHER_ALL
    aggs = [AggregateFunction("SUM", (Cast(Column(0), DataType.Float64),), DataType.Float64),
            AggregateFunction("SUM", (Cast(Column(2), DataType.Int32),), DataType.Int32)]
    for pred in (None, below(DataType.Float64)):
        rc, code, msg, src = _grouped_jit(US, pred, Cast(Column(0), DataType.Int64), aggs, flags)
        assert rc > 0, msg
        assert "dfmi::utf8_parse<i64>(A, 0, row, " in body_of(src)


def test_a_shape_without_a_new_cast_generates_the_same_source_with_and_without_the_flag():
    from test_jit_cpu import jit_check
    pred = BinaryExpr(BinaryExpr(Cast(Column(1), DataType.Float64), Operator.Divide, Column(3)), Operator.Gt,
                      Literal(Float64(3.0)))
    projs = [Cast(Column(3), DataType.Int32), Column(1)]
    for p, pr in ((pred, projs), (None, projs)):
        without = jit_check(US, p, pr, CAST | U8C)
        with_ = jit_check(US, p, pr, BOTH | U8C)
        assert without[0] > 0 and with_[0] > 0 and without[3] == with_[3]
        assert "utf8_parse" not in body_of(with_[3])


# ------------------------------------------------------------------- planning
TS = Schema([Field("s", DataType.Utf8, True), Field("b", DataType.Boolean, True)])
SQL = "SELECT CAST(s AS BIGINT), CAST(b AS INT) FROM t WHERE CAST(s AS DOUBLE) < 2.5"
DEBUG = ("Projection: CAST(#0 AS Int64), CAST(#1 AS Int32)\n"
         "  Selection: CAST(#0 AS Float64) Lt Float64(2.5)\n"
         "    TableScan: t projection=None")


def planned(flags=BOTH | _abi.DFMI_FLAG_EXT_GATHER_ALL):
    ctx = ExecutionContext(flags=flags)
    ctx.register_datasource("t", MemoryDataSource(TS, []))
    return ctx, SqlToRel(ctx).sql_to_rel(SQL)


def test_planning_and_compiling_the_plan():
    ctx, plan = planned()
    assert repr(plan) == DEBUG
    rel = ctx.execute(plan)  # compiles the predicate and the projections; nothing runs
    assert [f.data_type for f in rel.schema().fields] == [DataType.Int64, DataType.Int32]
    ctx0, plan0 = planned(CAST | _abi.DFMI_FLAG_EXT_GATHER_ALL)
    with pytest.raises(ExecutionError) as e:
        ctx0.execute(plan0)
    assert (e.value.kind, e.value.message) == ("NotImplemented", "CAST from Utf8 to Float64")


def test_serde_round_trip_of_the_plan():
    _, plan = planned()
    wire = serde.to_json(plan)
    back = serde.from_json(wire)
    assert repr(back) == DEBUG
    assert serde.to_json(back) == wire


# ------------------------------------------------------------ the host driver
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_parsers_under_asan_ubsan(tmp_path):
    skel = open(os.path.join(ROOT, "datafusion_amd", "csrc", "jit_skeleton.hip")).read()
    begin, end = "// ---- utf8 parse helpers: begin", "// ---- utf8 parse helpers: end"
    assert skel.count(begin) == 1 and skel.count(end) == 1
    helpers = skel[skel.index(begin):skel.index(end)]
    assert "Args" not in helpers.replace("no Args", "") and "__builtin_amdgcn" not in helpers
    for name in ("parse_int(", "parse_bool(", "parse_float(", "parse_big(", "parse_round("):
        assert name in helpers, name
    (tmp_path / "cast_parse_helpers.inc").write_text(helpers)
    out = str(tmp_path / "cast_parse_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", str(tmp_path), "-o", out,
           os.path.join(HERE, "native", "cast_parse_driver.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out, "100000"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "cast parse driver: clean" in r.stdout and "0 mismatches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
