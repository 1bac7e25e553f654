"""The carry normalisation of GROUP BY's exact sums on the device
(groupby.hip k_group_normalize, launched by agg_hash.cpp accumulate_hashed
once a state has absorbed 2^30 rows since the last pass), reached at test
sizes: DFMI_DIAG=1 DFMI_GROUP_NORM_ROWS=<n> lowers that threshold and
dfmi_internal_group_normalize_trips() counts the trips.

A carry pass rewrites every group's 68 signed 64-bit digits in place between
two batches. A wrong carry in the low digits disappears under the final
rounding unless the inputs cancel the high part away, so the table is built
for it (crafted_table): a borrow that ripples through all 68 digits, sums
past the finite range and back, the widest digit pieces in both signs, low
terms hidden under a high term that a later batch removes, groups of specials
and of NULLs only, a group that arrives after the last pass, random filler.
Every case compares keys, row counts and every value bit for bit with the
oracle over the concatenated table (its exact sums do not depend on batching;
it executes no AVG: SUM stands in its place and the AVG's bits come from the
contract restated on exact integers, tests/test_avg_cpu.py avg_bits) and with
the run that never normalises, and the trip counter with the rule restated in
rule_trips().

A carry pass moves value between digits and changes no sum: a pass that
skipped a digit, a sum or a group would finish to the same values. So the
cases also read the device records (dfmi_internal_group_records) before the
finish: the digits' value is the exact sum always, and right after a pass
over them -- the table's last batch adds two rows of NULLs to new groups --
they are the one normalised digit string of that sum.

tests/test_group_normalize_cpu.py checks the table and the oracle on the CPU
against exact rationals. No tolerance anywhere."""
import contextlib
import ctypes as C
import functools
import math
import os
import struct

import numpy as np
import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution.engine import engine, merge_grouped_partials, merge_grouped_partials_key_strings
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator
from oracle_ffi import oracle_aggregate_grouped_multi
from test_aggregate_cpu import agg, bits_f64, wild_doubles
from test_avg_cpu import F_NAN, F_NINF, F_NNZ, F_PINF, LIMBS, UNIT, avg_bits
from test_gpu_aggregate import slice_batch
from test_gpu_groupby_hash import _vals

pytestmark = pytest.mark.gpu

AGG = _abi.DFMI_FLAG_EXT_AGGREGATE | _abi.DFMI_FLAG_EXT_GATHER_ALL
FL = AGG | _abi.DFMI_FLAG_EXT_AGG_AVG
DMAX, FMAX = float(np.finfo(np.float64).max), float(np.finfo(np.float32).max)
Q64, Q32 = math.ldexp(1.0, -1074), math.ldexp(1.0, -149)  # the formats' quanta
NORM_ROWS = 1 << 30  # agg_state.h kGroupNormRows

# columns of every table here
KF, KS, KI, X, Y, V, SEL = range(7)
SCHEMA = Schema([Field("kf", DataType.Float64, True), Field("ks", DataType.Utf8, True), Field("ki", DataType.Int64, True),
                 Field("x", DataType.Float64, True), Field("y", DataType.Float32, True), Field("v", DataType.Int32, True),
                 Field("sel", DataType.Float64, False)])
# keys that go to the hash table, never the fused window kernel
KEYINGS = {"f64": [KF], "utf8": [KS], "i64": [KI], "i64_utf8": [KI, KS]}
# the float sums with integer aggregates between them: a wrong digit offset lands in a neighbour's words
AGGS = [("SUM", X), ("SUM", V), ("SUM", Y), ("MIN", V), ("AVG", X), ("MAX", V), ("AVG", Y), ("COUNT", X)]
NO_AVG = [("SUM", X), ("SUM", V), ("SUM", Y), ("COUNT", X)]
NO_FLOAT_SUM = [("SUM", V), ("MIN", V), ("MAX", V), ("COUNT", X), ("MIN", X)]


# ------------------------------------------------------------------ the tables
def wide64(k: int) -> float:
    """(2^53 - 1) * 2^(32k + 31 - 1074): shift 31 and an all-ones significand, the largest middle piece."""
    return math.ldexp(float(2 ** 53 - 1), 32 * k + 31 - 1074)


def wide32(k: int) -> float:
    return math.ldexp(float(2 ** 24 - 1), 4 * k - 149)


class Table:
    """Rows (batch, group id or -1 for the null key, x, y; None: NULL) as one
    host RecordBatch in batch order, the rows per batch, the groups by name."""

    def __init__(self, rows, names, seed, nbatches, sel_off=()):
        rng = np.random.default_rng(seed)
        order = []
        for b in range(nbatches):  # a batch's rows in random order: crafted groups between the filler's
            idx = [i for i, r in enumerate(rows) if r[0] == b]
            order += [idx[i] for i in rng.permutation(len(idx))]
        rows = [rows[i] for i in order]
        n = len(rows)
        self.n = n
        self.counts = [sum(1 for r in rows if r[0] == b) for b in range(nbatches)]
        self.gid = np.array([r[1] for r in rows], np.int64)
        self.x = [r[2] for r in rows]
        self.y = [None if r[3] is None else float(np.float32(r[3])) for r in rows]  # (as the Float32 column holds it)
        self.names = dict(names)  # name -> group id
        self.name_of = {g: nm for nm, g in self.names.items()}
        kv = self.gid >= 0
        xv, yv = np.array([v is not None for v in self.x]), np.array([v is not None for v in self.y])
        with np.errstate(over="ignore"):
            cols = [Array.from_numpy(DataType.Float64, self.gid * 0.5, kv),
                    Array.from_strings([self.name_of[g] if g >= 0 else None for g in self.gid]),
                    Array.from_numpy(DataType.Int64, (self.gid - 100) * 1_000_003, kv),
                    Array.from_numpy(DataType.Float64, np.array([0.0 if v is None else v for v in self.x]), xv),
                    Array.from_numpy(DataType.Float32, np.array([0.0 if v is None else v for v in self.y], np.float32), yv),
                    Array.from_numpy(DataType.Int32, rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32),
                                     rng.random(n) >= 0.1),
                    Array.from_numpy(DataType.Float64, np.array([1.0 if r[0] in sel_off else 0.0 for r in rows]))]
        self.sel = np.array([r[0] not in sel_off for r in rows])
        self.batch = RecordBatch(SCHEMA, cols)

    def starts(self):
        return [sum(self.counts[:b]) for b in range(len(self.counts) + 1)]

    def batches(self, device=True):
        """The explicit list of batches: views of the one table's buffers."""
        whole = self.batch.to(engine().device) if device else self.batch
        s = self.starts()
        return [slice_batch(whole, s[b], self.counts[b]) for b in range(len(self.counts))]

    @functools.lru_cache(maxsize=None)
    def exact(self, nrows=None, selected=False):
        """group id -> [x: (non-null values, exact sum of the finite ones in units of 2^-1074, flags), y: ...]
        over the first nrows rows (with `selected`: those the predicate sel < 0.5 keeps)."""
        out = {}
        for i in range(self.n if nrows is None else nrows):
            if selected and not self.sel[i]:
                continue
            e = out.setdefault(int(self.gid[i]), [[0, 0, 0], [0, 0, 0]])
            for c, v in enumerate((self.x[i], self.y[i])):
                if v is None:
                    continue
                e[c][0] += 1
                if v != v:
                    e[c][2] |= F_NAN
                elif v in (math.inf, -math.inf):
                    e[c][2] |= F_PINF if v > 0 else F_NINF
                else:
                    if not (v == 0 and math.copysign(1.0, v) < 0):
                        e[c][2] |= F_NNZ
                    e[c][1] += units(v)
        return out

    @functools.lru_cache(maxsize=None)
    def oracle(self, keying, aggs=tuple(AGGS), nrows=None, pred=False):
        b = self.batch if nrows is None else slice_batch(self.batch, 0, nrows)
        ref_aggs = [agg("SUM" if f == "AVG" else f, Column(c), SCHEMA) for f, c in aggs]
        return oracle_aggregate_grouped_multi(SCHEMA, b, PRED if pred else None, [Column(k) for k in KEYINGS[keying]],
                                              ref_aggs, AGG)


PRED = BinaryExpr(Column(SEL), Operator.Lt, Literal(Float64(0.5)))


def units(v: float) -> int:
    n, d = float(v).as_integer_ratio()
    return n * ((1 << UNIT) // d)


def sum_bits(total: int, n: int, f32: bool, flags: int):
    """The bits of SUM for an exact sum of `total` * 2^-1074 over n non-null values (None: null): avg_bits's
    contract with a divisor of 1, and a sum at or past the format's largest value plus half its last place is
    an infinity."""
    if n == 0:
        return None
    limit = (2 ** 128 - 2 ** 103 if f32 else 2 ** 1024 - 2 ** 970) << UNIT
    if not flags & (F_NAN | F_PINF | F_NINF) and abs(total) >= limit:
        return avg_bits(0, 1, f32, F_PINF if total > 0 else F_NINF)
    return avg_bits(total, 1, f32, flags)


def probe_rows(batch, first_gid):
    """A last batch that adds nothing to any digit: two rows of NULL arguments for two new groups far apart (an
    Int64 key of one value would take the key window). With DFMI_GROUP_NORM_ROWS=0 the pass before it leaves
    every record normalised."""
    return [(batch, first_gid, None, None), (batch, first_gid + 4000, None, None)], \
        {b"probe-a": first_gid, b"probe-b": first_gid + 4000}


@functools.lru_cache(maxsize=None)
def crafted_table() -> Table:
    """Batches A-D (0-3) and the probe batch E. Each crafted group's rows are spread so that a pass falls between
    them whether it runs before every batch or once before C. CRAFTED_WANT states the exact sums."""
    rows, names = [], {}

    def group(name, rs):
        g = len(names) + 1
        names[name] = g
        rows.extend((b, g, xv, yv) for b, xv, yv in rs)

    # the borrow of -2^-1074 ripples through all 68 digits: 0..66 at 0xffffffff, the top one -1
    group(b"ripple_zero", [(0, -Q64, -Q32), (2, Q64, Q32)])
    group(b"ripple_top", [(0, -Q64, -Q32), (1, Q64, Q32), (2, 2.0 ** 1023, 2.0 ** 127)])
    group(b"ripple_top_late", [(0, -Q64, -Q32), (2, Q64, Q32), (3, 2.0 ** 1023, 2.0 ** 127)])
    group(b"ripple_subnormal", [(0, -Q64, -Q32), (1, -Q64, -Q32), (3, -Q64, -Q32)])
    # the digits pass the finite range and come back
    group(b"over_and_back", [(0, DMAX, FMAX)] * 2 + [(1, -DMAX, -FMAX)] * 2 + [(1, 1.0, 1.0)])
    group(b"over_and_back_late", [(0, DMAX, FMAX)] * 2 + [(3, -DMAX, -FMAX)] * 2 + [(3, 1.0, 1.0)])
    group(b"over_and_stay", [(0, DMAX, FMAX), (1, DMAX, FMAX), (3, DMAX, FMAX)])
    group(b"over_negative", [(0, -DMAX, -FMAX)] * 2 + [(2, -DMAX, -FMAX)])
    # the widest pieces in both signs, cancelled later down to one small survivor
    for k in WIDE_K:
        for sg, tag in ((1.0, b"p"), (-1.0, b"m")):
            w, w32 = sg * wide64(k), sg * wide32(k)
            group(b"widest_%d" % k + tag, [(0, w, w32)] * 3 + [(2, -w, -w32)] + [(3, -w, -w32)] * 2 +
                  [(3, sg * (k + 1) * Q64, sg * (k + 1) * Q32)])
    # low digits hidden under a high term until a later batch removes it
    group(b"hidden_low", [(0, 2.0 ** 60, 2.0 ** 30), (0, 2.0 ** -1000, 2.0 ** -100), (2, -2.0 ** 60, -2.0 ** 30)])
    group(b"hidden_low_negative", [(0, 2.0 ** 60, 2.0 ** 30), (0, -2.0 ** -1000, -2.0 ** -100),
                                   (2, -2.0 ** 60, -2.0 ** 30)])
    group(b"hidden_chain", [(0, 2.0 ** 900, 2.0 ** 100), (1, -2.0 ** 900, -2.0 ** 100), (1, 2.0 ** 700, 2.0 ** 40),
                            (2, -2.0 ** 700, -2.0 ** 40), (2, 2.0 ** 500, 2.0 ** -20), (3, -2.0 ** 500, -2.0 ** -20),
                            (3, 2.0 ** 300, 2.0 ** -80)])
    # specials only: the digits stay zero, the flags and the non-zero count survive
    inf, nan = math.inf, math.nan
    group(b"special_pinf", [(0, inf, inf), (2, 0.0, 0.0), (3, -0.0, -0.0)])
    group(b"special_ninf", [(0, -inf, -inf), (3, -inf, -inf)])
    group(b"special_both_inf", [(0, inf, inf), (1, -inf, -inf), (3, 0.0, 0.0)])
    group(b"special_nan", [(0, nan, nan), (2, -0.0, -0.0), (3, inf, inf)])
    group(b"special_negative_zero", [(0, -0.0, -0.0), (1, -0.0, -0.0), (3, -0.0, -0.0)])
    group(b"special_zeros", [(0, -0.0, -0.0), (2, 0.0, 0.0), (3, -0.0, -0.0)])
    group(b"nulls_only", [(0, None, None), (1, None, None), (3, None, None)])
    group(b"nulls_and_one_value", [(0, None, 1.5), (1, 2.5, None), (3, None, None)])
    # many rows of one group in a batch: the wave-summed leader add, the bucketed LDS record
    a, a32, c, c32 = wide64(31), wide32(31), wide64(40), wide32(40)
    group(b"heavy", [(0, a, a32)] * 130 + [(2, -a, -a32)] * 130 + [(2, -c, -c32)] * 130 + [(3, c, c32)] * 130 +
          [(3, 5 * Q64, 5 * Q32)])
    # a first row in the last batch that adds rows: the pass before it ran over a table without the group
    group(b"late_arrival", [(3, -3.0e300, -3.0e30), (3, 1.0e-300, 1.0e-30), (3, 3.0e300, 3.0e30)])
    # filler: a few hundred random groups, rows in every batch, 10% NULLs, the null key too
    rng = np.random.default_rng(20_26)
    fill = 300
    for f in range(fill):
        group(b"f%04d" % f if f % 50 else b"filler with a key longer than the slot's 24 bytes %04d" % f, [])
    first = len(names) - fill + 1
    for b, nb in enumerate((1500, 1200, 1000, 900)):
        xs = wild_doubles(rng, nb)
        ys = (rng.standard_normal(nb) * np.exp2(rng.integers(-140, 120, nb))).astype(np.float32)
        gs = rng.integers(first - 1, first + fill, nb)  # (first - 1: the null key)
        for i in range(nb):
            rows.append((b, -1 if gs[i] < first else int(gs[i]), None if rng.random() < 0.1 else float(xs[i]),
                         None if rng.random() < 0.1 else float(ys[i])))
    pr, pn = probe_rows(4, len(names) + 1)
    names.update(pn)
    return Table(rows + pr, names, 1, 5)


WIDE_K = (0, 1, 2, 17, 33, 61, 62)
# the exact SUM(x), SUM(y) the crafted groups are built to have (None: NULL)
CRAFTED_WANT = {
    b"ripple_zero": (0.0, 0.0), b"ripple_top": (2.0 ** 1023, 2.0 ** 127), b"ripple_top_late": (2.0 ** 1023, 2.0 ** 127),
    b"ripple_subnormal": (-3 * Q64, -3 * Q32), b"over_and_back": (1.0, 1.0), b"over_and_back_late": (1.0, 1.0),
    b"over_and_stay": (math.inf, math.inf), b"over_negative": (-math.inf, -math.inf),
    b"hidden_low": (2.0 ** -1000, 2.0 ** -100), b"hidden_low_negative": (-2.0 ** -1000, -2.0 ** -100),
    b"hidden_chain": (2.0 ** 300, 2.0 ** -80), b"special_pinf": (math.inf, math.inf),
    b"special_ninf": (-math.inf, -math.inf), b"special_both_inf": (math.nan, math.nan),
    b"special_nan": (math.nan, math.nan), b"special_negative_zero": (-0.0, -0.0), b"special_zeros": (0.0, 0.0),
    b"nulls_only": (None, None), b"nulls_and_one_value": (2.5, 1.5), b"heavy": (5 * Q64, 5 * Q32),
    b"late_arrival": (1.0e-300, float(np.float32(1.0e-30))),
    b"probe-a": (None, None), b"probe-b": (None, None),
}
for _k in WIDE_K:
    CRAFTED_WANT[b"widest_%dp" % _k] = ((_k + 1) * Q64, (_k + 1) * Q32)
    CRAFTED_WANT[b"widest_%dm" % _k] = (-(_k + 1) * Q64, -(_k + 1) * Q32)


@functools.lru_cache(maxsize=None)
def high_low_table(first: int, more: int, sel_off=()) -> Table:
    """Groups whose high term hides a negative low one until a later batch removes the high term. Batch 0: groups
    [0, first) get +H and a low term; batch 1: `more` new groups get the same and the first lose their H; batch
    2: the new groups lose their H, the first get a second low term; batch 3: the probe rows. Every record holds
    a negative digit before each pass, whichever group is the table's last."""
    rows, names = [], {}
    for g in range(first + more):
        names[b"g%06d" % g] = g + 1
        low, low32 = -(g + 1) * math.ldexp(1.0, -1074 + 17 * (g % 50)), -(g + 1) * math.ldexp(1.0, -149 + 3 * (g % 40))
        b0 = 0 if g < first else 1
        rows += [(b0, g + 1, 2.0 ** 900, 2.0 ** 100), (b0, g + 1, low, low32), (b0 + 1, g + 1, -2.0 ** 900, -2.0 ** 100)]
        if g < first:
            rows.append((2, g + 1, low * 3, low32 * 3))
    pr, pn = probe_rows(3, first + more + 1)
    names.update(pn)
    return Table(rows + pr, names, 2, 4, sel_off)


# ------------------------------------------------------------- the device side
@contextlib.contextmanager
def diag(**knobs):
    """DFMI_DIAG=1 and the given knobs (None: unset) for the block; the environment as it was afterwards."""
    knobs = dict(knobs, DFMI_DIAG="1")
    old = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


FINISH = {"device": {}, "host": {"DFMI_GROUP_HOST_FINISH": "1"}, "emit0": {"DFMI_GROUP_DEVICE_EMIT": "0"},
          "emit1": {"DFMI_GROUP_DEVICE_EMIT": "1"}}


def trips() -> int:
    f = _abi.lib().dfmi_internal_group_normalize_trips
    f.restype = C.c_long
    return f()


def rule_trips(ms, threshold, float_sum=True, r=0):
    """accumulate_hashed's rule restated: (trips, rows since the last pass) after batches of `ms` selected rows."""
    t = 0
    for m in ms:
        if m > 0:
            if float_sum and r + m > threshold:
                t, r = t + 1, 0
            r += m
    return t, r


def new_state(keying, aggs=AGGS):
    cs = [compile_expr(None, agg(f, Column(c), SCHEMA), SCHEMA, FL) for f, c in aggs]
    ks = [compile_scalar_expr(None, Column(k), SCHEMA, FL) for k in KEYINGS[keying]]
    return engine().grouped_agg_state(ks, cs), cs


def add_batches(st, batches, pred=None, many=None):
    """The driver: the explicit list of batches added to one state, one add() each, or (`many`: sizes) in
    consecutive coalesced calls of that many batches."""
    p = compile_scalar_expr(None, pred, SCHEMA, FL) if pred is not None else None
    if many is None:
        for b in batches:
            st.add(p, b, FL)
        return
    assert sum(many) == len(batches)
    b0 = 0
    for k in many:
        st.add_many(p, batches[b0:b0 + k], FL)
        b0 += k


def records(st, g0=0, ng=None):
    """The device records of groups [g0, g0 + ng) as they stand: ([ng][words] int64, the float sums' digit offsets)."""
    st.eng.drain()
    f = _abi.lib().dfmi_internal_group_records
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    info = np.zeros(3 + 15, np.int64)
    err = _abi.dfmi_error()
    assert f(st.eng.ctx, st.handle, 0, 0, None, info.ctypes.data, C.addressof(err)) == _abi.DFMI_OK
    words, held, nf = int(info[0]), int(info[1]), int(info[2])
    if ng is None:
        ng = held - g0
    out = np.zeros((ng, max(words, 1)), np.int64)
    assert f(st.eng.ctx, st.handle, g0, ng, out.ctypes.data, info.ctypes.data, C.addressof(err)) == _abi.DFMI_OK, \
        err.message
    return out, [int(o) for o in info[3:3 + nf]]


def digits_of(total: int):
    """The one normalised digit string of `total`: 67 digits in [0, 2^32), the top one signed."""
    d = []
    for _ in range(LIMBS - 1):
        d.append(total & 0xffffffff)
        total >>= 32  # floor
    return tuple(d) + (total,)


def value_of(d) -> int:
    return sum(int(x) << (32 * i) for i, x in enumerate(d))


def check_records(t: Table, st, aggs, normalised: bool, nrows=None, selected=False):
    """The device records against the table's exact sums, as multisets over the groups (the records lie in claim
    order): each float sum's digits have the exact sum's value; `normalised` (a pass ran over them and nothing
    was added since): they are its normalised digit string. Returns whether any digit lay outside [0, 2^32)."""
    rec, foff = records(st)
    cols = [c for f, c in aggs if f in ("SUM", "AVG") and c in (X, Y)]
    assert len(foff) == len(cols)
    ex = t.exact(nrows, selected)
    assert len(rec) == len(ex)
    small = len(rec) <= 4000  # (tens of thousands of groups: the digits' range and the sums' signs only)
    if small:
        want = sorted(tuple(e[c - X][1] for c in cols) for e in ex.values())
        got = sorted(tuple(value_of(r[o:o + LIMBS]) for o in foff) for r in rec)
        assert got == want
    low = np.stack([rec[:, o:o + LIMBS - 1] for o in foff])
    loose = bool(((low < 0) | (low >= 2 ** 32)).any())
    if normalised:
        assert not loose
        top = np.stack([rec[:, o + LIMBS - 1] for o in foff], axis=1)
        assert sorted(tuple(int(x) for x in r) for r in top) == \
            sorted(tuple(e[c - X][1] >> (32 * (LIMBS - 1)) for c in cols) for e in ex.values())
    if normalised and small:
        assert sorted(tuple(tuple(int(x) for x in r[o:o + LIMBS]) for o in foff) for r in rec) == \
            sorted(tuple(digits_of(e[c - X][1]) for c in cols) for e in ex.values())
    return loose


def plain(st, out, nkeys):
    """A finish's result as plain tuples: keys, Utf8 key bytes, values."""
    dk, dv = out
    keys = [[(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in g] for g in dk]
    strs = [st.key_strings(p) if len(keys) and keys[0][p][0] == int(DataType.Utf8) else None for p in range(nkeys)]
    return keys, strs, [[(int(v.type), int(v.is_null), int(v.count), 0 if v.is_null else int(v.bits)) for v in g]
                        for g in dv]


def group_ids(t: Table, keying, rk, rs):
    """The table's group id of each of the oracle's groups."""
    ids = []
    for g, parts in enumerate(rk):
        if keying == "utf8":
            ids.append(-1 if rs[0][g] is None else t.names[rs[0][g]])
        elif parts[0].is_null:
            ids.append(-1)
        elif keying == "f64":
            ids.append(int(struct.unpack("<d", struct.pack("<Q", int(parts[0].bits)))[0] * 2))
        else:
            b = int(parts[0].bits)
            ids.append((b - (1 << 64) if b >> 63 else b) // 1_000_003 + 100)
    return ids


def check_oracle(t: Table, keying, got, aggs=AGGS, nrows=None, pred=False):
    """`got` (plain()) against the oracle over the first nrows rows: keys, Utf8 bytes, row counts, values; an AVG's
    type, null flag and count are those of the oracle's SUM in its place, its bits the restatement's."""
    rk, rv, rs = t.oracle(keying, tuple(aggs), nrows, pred)
    keys, strs, vals = got
    assert len(keys) == len(rk)
    assert keys == [[(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in g] for g in rk]
    for p, s in enumerate(rs):
        if s is not None:
            assert strs[p] == s, p
    ids = group_ids(t, keying, rk, rs)
    ex = t.exact(nrows, pred)
    assert sorted(ids) == sorted(ex)
    for g in range(len(rk)):
        ref = _vals(rv[g])
        for j, (f, c) in enumerate(aggs):
            r = (int(ref[j][0]), int(ref[j][1]), int(ref[j][2]), int(ref[j][3]))
            if f == "AVG":
                assert not pred  # (a filtered batch has no validity: the restatement reads the table's)
                n, total, flags = ex[ids[g]][c - X]
                want = avg_bits(total, n, c == Y, flags)
                r = r[:3] + (0 if want is None else want,)
                assert n == r[2] and (want is None) == bool(r[1])
            assert vals[g][j] == r, (g, ids[g], t.name_of.get(ids[g]), j, f)


def run(t: Table, keying, env, aggs=AGGS, many=None, pred=False, check_digits=True, normalised=None):
    """One state over the table's batches under the knobs `env`: (plain result, trips counted, whether a digit
    lay outside [0, 2^32) before the finish). The records are checked before the finish (`normalised`: a pass ran
    right before the probe batch -- by default with DFMI_GROUP_NORM_ROWS=0), the result against the oracle."""
    if normalised is None:
        normalised = env.get("DFMI_GROUP_NORM_ROWS") == "0"
    with diag(**env):
        st, _ = new_state(keying, aggs)
        t0 = trips()
        add_batches(st, t.batches(), PRED if pred else None, many)
        counted = trips() - t0
        loose = None
        if check_digits:
            loose = check_records(t, st, aggs, normalised, None, pred)
        got = plain(st, st.finish(), len(KEYINGS[keying]))
    check_oracle(t, keying, got, aggs, None, pred)
    return got, counted, loose


def env_of(norm, buckets, finish, t: Table):
    env = dict(FINISH[finish], DFMI_GROUP_BUCKETS=buckets)
    if norm is not None:
        # "mid": the rows of the first two batches -- the threshold trips once, before the third
        env["DFMI_GROUP_NORM_ROWS"] = "0" if norm == "0" else str(t.counts[0] + t.counts[1])
    return env


@functools.lru_cache(maxsize=None)
def unforced(keying, buckets, finish):
    """The crafted table through a state that never normalises (the knob unset): the counter stays, the digits
    really are loose before the finish, the result equals the oracle's."""
    t = crafted_table()
    got, counted, loose = run(t, keying, env_of(None, buckets, finish, t))
    assert counted == 0 and loose
    return got


CASES = [(k, f) for k in KEYINGS for f in (("device", "host", "emit0", "emit1") if k == "f64" else ("device", "host"))]


# ------------------------------------------------------------------- the tests
@pytest.mark.parametrize("buckets", ["0", "1"])
@pytest.mark.parametrize("norm", ["0", "mid"])
@pytest.mark.parametrize("keying,finish", CASES)
def test_crafted_batches(keying, finish, norm, buckets):
    """The crafted table, a pass before every batch ("0": 5 trips) or once before batch C ("mid": 1 trip), through
    the atomic and the bucketed passes and each finish: equal to the oracle, to the unforced run, the counter to
    the rule, the records' digits to the exact sums' (normalised after the last pass with "0")."""
    t = crafted_table()
    env = env_of(norm, buckets, finish, t)
    want_trips, _ = rule_trips(t.counts, int(env["DFMI_GROUP_NORM_ROWS"]))
    assert want_trips == (5 if norm == "0" else 1)
    assert rule_trips(t.counts, NORM_ROWS)[0] == 0
    got, counted, loose = run(t, keying, env)
    assert counted == want_trips
    assert got == unforced(keying, buckets, finish)
    assert loose == (norm != "0")
    # the specials really occur among the results
    sx = {v[0][3] for v in got[2] if not v[0][1]}
    sy = {v[2][3] for v in got[2] if not v[2][1]}
    assert 0 in sx and 0x8000000000000000 in sx and 0x7FF0000000000000 in sx and 0xFFF0000000000000 in sx
    assert bits_f64(-3 * Q64) in sx and bits_f64(5 * Q64) in sx and 0x7FF8000000000000 in sx  # subnormals, NaN
    assert 0 in sy and 0x80000000 in sy and 0x7F800000 in sy and 0xFF800000 in sy and 0x80000003 in sy
    assert any(v[0][1] for v in got[2])  # a NULL sum


@pytest.mark.parametrize("buckets", ["0", "1"])
@pytest.mark.parametrize("keying", ["f64", "utf8", "i64_utf8"])
def test_partial_after_forced_normalisation(keying, buckets):
    """The grouped partial carries each group's exact digits, not a rounded value: after a pass before every batch
    it is byte-identical to the unforced state's, and merged it equals the oracle."""
    t = crafted_table()
    parts = []
    for norm in (None, "0"):
        with diag(**env_of(norm, buckets, "device", t)):
            st, cs = new_state(keying)
            t0 = trips()
            add_batches(st, t.batches())
            assert trips() - t0 == (5 if norm else 0)
            parts.append(st.partial())
    assert parts[0] == parts[1]
    nk = len(KEYINGS[keying])
    mk, mv = merge_grouped_partials(cs, [parts[1]], nk, True)
    keys = [[(int(k.type), int(k.is_null), int(k.bits), int(k.count)) for k in g] for g in mk]
    strs = []
    for p in range(nk):
        strs.append(None)
        if KEYINGS[keying][p] == KS:
            s = merge_grouped_partials_key_strings(cs, [parts[1]], p, len(mk))
            strs[p] = [None if keys[g][p][1] else s[g] for g in range(len(mk))]
    vals = [[(int(v.type), int(v.is_null), int(v.count), 0 if v.is_null else int(v.bits)) for v in g] for g in mv]
    check_oracle(t, keying, (keys, strs, vals))


@pytest.mark.parametrize("finish", ["device", "host"])
@pytest.mark.parametrize("keying", ["f64", "utf8"])
def test_state_life_cycle(keying, finish):
    """DFMI_GROUP_NORM_ROWS=0 over a state's life: finish, more rows, finish again (each prefix equal to the
    oracle's); reset and the same again. Then the rule's row count: it restarts from 0 at a reset -- with the
    threshold at the first two batches' rows, those two never trip after a reset, the third does."""
    t = crafted_table()
    b, s = t.batches(), t.starts()
    nk = len(KEYINGS[keying])
    with diag(DFMI_GROUP_NORM_ROWS="0", **FINISH[finish]):
        st, _ = new_state(keying)
        for _ in range(2):
            t0 = trips()
            add_batches(st, b[:2])
            check_oracle(t, keying, plain(st, st.finish(), nk), nrows=s[2])
            add_batches(st, b[2:3])
            check_oracle(t, keying, plain(st, st.finish(), nk), nrows=s[3])
            check_oracle(t, keying, plain(st, st.finish(), nk), nrows=s[3])
            add_batches(st, b[3:])
            check_oracle(t, keying, plain(st, st.finish(), nk))
            assert trips() - t0 == 5
            st.reset()
            assert len(st.finish()[0]) == 0
    threshold = t.counts[0] + t.counts[1]
    with diag(DFMI_GROUP_NORM_ROWS=threshold, **FINISH[finish]):
        t0 = trips()
        add_batches(st, b[:2])
        assert trips() - t0 == 0 == rule_trips(t.counts[:2], threshold)[0]
        st.reset()
        add_batches(st, b[:2])
        assert trips() - t0 == 0  # (without the restart the first batch would trip: 2 * counts[0] + counts[1] rows)
        assert rule_trips(t.counts[:2] + t.counts[:1], threshold)[0] == 1
        add_batches(st, b[2:])
        assert trips() - t0 == 1 == rule_trips(t.counts, threshold)[0]
        check_oracle(t, keying, plain(st, st.finish(), nk))


@pytest.mark.parametrize("buckets", ["0", "1"])
@pytest.mark.parametrize("keying", ["f64", "i64_utf8"])
def test_records_regrown_between_passes(keying, buckets):
    """600 groups, then 900 more: the record array (1,024 records at first) is regrown in the batch whose pass
    normalises the first 600. Every record holds a negative digit before each pass, so a pass that skipped one
    group -- the last, say -- leaves it outside [0, 2^32): the digits are checked after the last pass."""
    t = high_low_table(600, 900)
    got, counted, loose = run(t, keying, {"DFMI_GROUP_NORM_ROWS": "0", "DFMI_GROUP_BUCKETS": buckets})
    assert counted == 4 == rule_trips(t.counts, 0)[0] and not loose
    base, counted, loose = run(t, keying, {"DFMI_GROUP_BUCKETS": buckets})
    assert counted == 0 and loose and got == base
    assert len(got[0]) == 1502


def test_table_growth_between_passes():
    """17,000 groups, then 16,000 more: the claim pass overflows the first 65,536-slot table (at half full), which
    is grown and rehashed in the batch whose pass normalises the first 17,000 (at this size the records' digits
    are checked for their range and sign, their values by the finish alone)."""
    t = high_low_table(17_000, 16_000)
    got, counted, loose = run(t, "f64", {"DFMI_GROUP_NORM_ROWS": "0"})
    assert counted == 4 and not loose and len(got[0]) == 33_002


def test_batch_that_selects_nothing_is_no_trip():
    """The predicate keeps no row of batch 1: accumulate_hashed returns before the threshold is looked at. Three
    trips for four batches with DFMI_GROUP_NORM_ROWS=0; with the threshold at batch 0's rows plus one, batch 2
    trips as it would right after batch 0."""
    t = high_low_table(300, 200, sel_off=(1,))
    ms = [t.counts[0], 0, t.counts[2], t.counts[3]]
    got, counted, loose = run(t, "f64", {"DFMI_GROUP_NORM_ROWS": "0"}, NO_AVG, pred=True)
    assert counted == 3 == rule_trips(ms, 0)[0] and not loose
    base, counted, _ = run(t, "f64", {}, NO_AVG, pred=True)
    assert counted == 0 and got == base
    mid = t.counts[0] + 1
    _, counted, _ = run(t, "f64", {"DFMI_GROUP_NORM_ROWS": str(mid)}, NO_AVG, pred=True)
    assert counted == rule_trips(ms, mid)[0] == 1 and rule_trips(t.counts, mid)[0] == 2


@pytest.mark.parametrize("many", [(2, 2, 1), (3, 2)])
@pytest.mark.parametrize("norm", ["0", "mid"])
@pytest.mark.parametrize("keying", ["f64", "i64", "utf8"])
def test_coalesced_calls(keying, norm, many):
    """The crafted batches through add_many (dfmi_aggregate_batches) in calls of 2 and of 3 batches. A coalesced
    call with fixed-width keys runs the table's passes once over its packed rows: the rule sees one m per call,
    the sum of its batches' rows. A state with a Utf8 key takes the call's batches one by one: one m per batch."""
    t = crafted_table()
    env = env_of(norm, "0", "device", t)
    ms, b0 = [], 0
    for k in many:
        ms.append(sum(t.counts[b0:b0 + k]))
        b0 += k
    if keying == "utf8":
        ms = t.counts
    want_trips = rule_trips(ms, int(env["DFMI_GROUP_NORM_ROWS"]))[0]
    # "mid" (the threshold at A's and B's rows): a call of A, B and C trips by itself, over the table without a
    # group, and the call after it again
    assert want_trips == (len(ms) if norm == "0" else 2 if len(ms) == 2 else 1)
    # the records are normalised before the finish where the probe batch is a pass's only batch: with "0", alone
    # in its call or one by one; in a call with D the pass runs before D's rows
    normalised = norm == "0" and (keying == "utf8" or many[-1] == 1)
    got, counted, loose = run(t, keying, env, many=list(many), normalised=normalised)
    assert counted == want_trips
    assert loose == (not normalised)
    assert got == unforced(keying, "0", "device")


def test_state_without_float_sums_never_trips():
    """Integer SUM / MIN / MAX, COUNT and a float MIN hold no digits: the threshold is not looked at."""
    t = crafted_table()
    got, counted, _ = run(t, "f64", {"DFMI_GROUP_NORM_ROWS": "0"}, NO_FLOAT_SUM, check_digits=False)
    assert counted == 0 == rule_trips(t.counts, 0, float_sum=False)[0]
    base, _, _ = run(t, "f64", {}, NO_FLOAT_SUM, check_digits=False)
    assert got == base


def test_grid_stride_loop_past_one_launch():
    """8 float sums over 2^18 + 5 groups: 2,097,192 digit strings for the launch's 8,192 x 256 threads, so the
    last five groups' are reached by the grid-stride step only. Batch 0 gives every group and sum a high term
    and a negative low term of its own, the pass before batch 1 normalises them, batch 1 removes the high terms,
    the pass before the probe batch normalises again: the finished values against the oracle's, the last
    groups' against the low terms themselves, and the first and last 1,024 records' digits (no partial here)."""
    ng, ns = (1 << 18) + 5, 8
    assert ng * ns > 8192 * 256 == (ng - 5) * ns
    g = np.arange(ng, dtype=np.int64)
    high = [2.0 ** (900 - 40 * j) if j % 2 == 0 else 2.0 ** (100 - 8 * j) for j in range(ns)]
    low = [-(g + 1 + j).astype(np.float64) * np.exp2(-1074.0 + (g % 32) + j) if j % 2 == 0
           else -(g + 1 + j).astype(np.float64) * np.exp2(-149.0 + (g % 16) + j) for j in range(ns)]
    probe = np.array([ng + 10, ng + 5000], np.int64)
    # (a Float64 key: the hash table alone; eight float sums are past the window kernel's four)
    key = np.concatenate([g, g, g, probe]) * 0.5
    n = len(key)
    valid = np.ones(n, bool)
    valid[-2:] = False
    fields, cols = [Field("k", DataType.Float64, False)], [Array.from_numpy(DataType.Float64, key)]
    for j in range(ns):
        ty, nt = (DataType.Float64, np.float64) if j % 2 == 0 else (DataType.Float32, np.float32)
        vals = np.concatenate([np.full(ng, high[j]), low[j], np.full(ng, -high[j]), np.zeros(2)]).astype(nt)
        assert np.array_equal(vals[ng:2 * ng].astype(np.float64), low[j])  # (exact in the column's type)
        fields.append(Field("c%d" % j, ty, True))
        cols.append(Array.from_numpy(ty, vals, valid))
    s = Schema(fields)
    whole = RecordBatch(s, cols)
    aggs_e = [agg("SUM", Column(1 + j), s) for j in range(ns)]
    counts = [2 * ng, ng, 2]
    with diag(DFMI_GROUP_NORM_ROWS="0"):
        st = engine().grouped_agg_state([compile_scalar_expr(None, Column(0), s, FL)],
                                        [compile_expr(None, a, s, FL) for a in aggs_e])
        dev = whole.to(engine().device)
        t0 = trips()
        for r0, m in zip((0, 2 * ng, 3 * ng), counts):
            st.add(None, slice_batch(dev, r0, m), FL)
        assert trips() - t0 == 3 == rule_trips(counts, 0)[0]
        for g0 in (0, ng - 1024):
            rec, foff = records(st, g0, 1024)
            assert len(foff) == ns
            lowd = np.stack([rec[:, o:o + LIMBS - 1] for o in foff])
            assert not ((lowd < 0) | (lowd >= 2 ** 32)).any()
            assert (np.stack([rec[:, o + LIMBS - 1] for o in foff]) == -1).all()  # (every sum is negative)
        dk, dv = st.finish()
    assert len(dk) == ng + 2
    assert np.array_equal(dk["bits"][:, 0], (np.concatenate([g, probe]) * 0.5).view(np.uint64))
    for j in range(ns):
        want = low[j].view(np.uint64) if j % 2 == 0 else low[j].astype(np.float32).view(np.uint32).astype(np.uint64)
        assert np.array_equal(dv["bits"][:ng, j], want), j
        assert [int(x) for x in dv["bits"][ng - 5:ng, j]] == [int(x) for x in want[-5:]]
        assert (dv["is_null"][:ng, j] == 0).all() and (dv["is_null"][ng:, j] == 1).all()
    rk, rv, _ = oracle_aggregate_grouped_multi(s, whole, None, [Column(0)], aggs_e, AGG)
    assert len(rk) == ng + 2
    ref = np.array([[(v.type, v.is_null, v.count, 0 if v.is_null else v.bits) for v in grp] for grp in rv], np.uint64)
    got = np.stack([dv[f].astype(np.uint64) for f in ("type", "is_null", "count", "bits")], axis=-1)  # (exact in uint64)
    got[..., 3][got[..., 1] != 0] = 0
    assert np.array_equal(got, ref)
    assert [(int(k[0].is_null), int(k[0].bits), int(k[0].count)) for k in rk] == \
        [(int(a), int(b), int(c)) for a, b, c in zip(dk["is_null"][:, 0], dk["bits"][:, 0], dk["count"][:, 0])]
