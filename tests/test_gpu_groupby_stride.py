"""The GROUP BY and Utf8 MIN / MAX kernels past one grid of workgroups.

Every kernel of groupby.hip and str_extreme.hip but k_group_scan and
k_group_bucket is a grid-stride or tile-stride loop over a capped grid
(groupby.h "Diagnostic grid cap"): 8192 blocks of 256 for the row, slot, group
and record passes, 1024 blocks of 4,096-row tiles for the rank and scatter
passes, 2048 for k_group_concat / k_group_bits_to_u8, 1024 (512 for
k_sx_prefix_one) for the string passes. The rest of the suite stops at or
below one trip of every loop over rows, slots and groups. Over
test_gpu_groupby_hash.py, test_gpu_minmax_any.py, test_gpu_agg_batches.py,
test_gpu_group_normalize.py and test_gpu_avg.py
dfmi_internal_group_strided_launches() counts 16 launches, all over record
words: k_group_init growing the records of 24,000 groups and more past
2,097,152 words, and the carry pass and the finish of 2^18 + 5 groups in
test_grid_stride_loop_past_one_launch. So a block's bucket cursors carried
from tile to tile, several tiles in one LDS histogram, the wave ballots and
the wave-aggregated group ids on a later, partial trip, the rehash, and the
group-strided passes of the compaction, the emission and the string side ran
nowhere but in the benchmark.

Forced shape: DFMI_DIAG=1 DFMI_GROUP_GRID=3 (an odd count: uneven shares) and
N = 5 x 4096 + 77 = 20,557 rows per batch. Rank and scatter: six tiles over
three blocks, two each, the last of 77 rows. Claim and accumulate: 27 trips of
768 rows, the last of 589 -- two full blocks, then one full wave and a wave of
13 lanes. Production shape: 2^22 + 3 x 4096 + 77 rows with no knob, the
shipped grids on their second and third trips.

Every case compares every group with the oracle bit for bit -- keys, Utf8 key
bytes, row counts, values, winning strings -- through the helpers of the files
named above, and asserts that the strided-launch counter rose: the counter
proves the loops ran, the oracle that they are right."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_agg_batches as tb
import test_gpu_minmax_any as mm
from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution.engine import engine
from datafusion_amd.execution.expression import compile_expr, compile_scalar_expr
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator
from oracle_ffi import oracle_aggregate_grouped_multi
from test_aggregate_cpu import agg, wild_doubles
from test_gpu_aggregate import slice_batch
from test_gpu_avg import Table, exprs
from test_gpu_group_normalize import trips
from test_gpu_groupby_hash import AGGS, FL, _bucketed_batches, _table, run_multi

pytestmark = pytest.mark.gpu

N = 5 * 4096 + 77  # rows per batch: six scatter tiles, 27 trips of 3 x 256 rows
GRID = "3"
assert N == 26 * 768 + 589 and 589 == 2 * 256 + 64 + 13


def strided() -> int:
    f = _abi.lib().dfmi_internal_group_strided_launches
    f.restype = C.c_long
    return f()


@contextlib.contextmanager
def strides(what):
    """The block launched at least one kernel that took more than one trip of its grid."""
    before = strided()
    yield
    print("strided launches, %s: +%d" % (what, strided() - before))
    assert strided() > before, what


@pytest.fixture
def grid3(monkeypatch):
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_GROUP_GRID", GRID)
    return monkeypatch


def head(b: RecordBatch, n: int) -> RecordBatch:
    return slice_batch(b, 0, n)


# ------------------------------------------------ atomic and bucketed passes
KEYSETS = {"int64": [Column(0)], "int64_utf8": [Column(0), Column(1)], "boolean": [Column(3)],
           "boolean_twice": [Column(3), Column(3)], "three": [Column(3), Column(2), Column(0)],
           "four": [Column(1), Column(3), Column(2), Column(0)]}
# One Boolean key is the key-window kernel's (aggregate.cpp: keys always [false, true]), whatever DFMI_GROUP_BUCKETS
# says: that state never reaches the hash table, so it launches nothing of groupby.hip and moves neither counter.
# The same three groups with every lane on the same few records reach it as a two-part key.
WINDOW = ("boolean",)
# Thousands of groups of two and four parts (the oracle's and the comparison's time): three batches without a
# predicate and one with; the other key sets run all four combinations.
MANY_GROUPS = ("int64_utf8", "four")
PRED = BinaryExpr(Column(4), Operator.Lt, Literal(Float64(0.6)))


@functools.lru_cache(maxsize=None)
def wide_table():
    """test_gpu_groupby_hash._table over three batches of N rows: nullable Int64, Utf8, Float64 and Boolean key
    parts; wild doubles and Int32 arguments with nulls."""
    return _table(np.random.default_rng(901), 3 * N)


@functools.lru_cache(maxsize=None)
def wide_ref(keyset: str, with_pred: bool, rows: int):
    """The oracle's groups over the first `rows` rows, once for every device run that shares them."""
    s, b = wide_table()
    return oracle_aggregate_grouped_multi(s, head(b, rows), PRED if with_pred else None, KEYSETS[keyset], AGGS(s), FL, 0)


@pytest.mark.parametrize("keyset", list(KEYSETS))
@pytest.mark.parametrize("buckets", ["0", "1"])
def test_forced_grid_atomic_and_bucketed_passes(grid3, buckets, keyset):
    """k_group_claim + k_group_accumulate (DFMI_GROUP_BUCKETS=0) and k_group_rank / _rank_fixed + k_group_scatter
    (=1) at three workgroups: one batch of N rows, and three batches into one state -- in the later ones the
    persisted-key comparisons run on later trips and tiles, and the accumulators, the table and the key arena
    carry over -- with and without a predicate; Float64 SUM over wild doubles, COUNT, Float64 MIN, Int32 MAX and SUM
    over nullable arguments; one Int64 key, (Int64, Utf8), a Boolean key (3 groups: every lane of a wave on the same
    few records: the Boolean key, twice over so that the hash table takes it -- the single Boolean key is the window
    kernel's and only checked against the oracle) and three and four key parts."""
    grid3.setenv("DFMI_GROUP_BUCKETS", buckets)
    s, b = wide_table()
    keys = KEYSETS[keyset]
    hashed = keyset not in WINDOW
    before = _bucketed_batches()
    runs = [(False, N, 0), (False, 3 * N, N), (True, N, 0), (True, 3 * N, N)]
    for with_pred, rows, batch_rows in runs[1:3] if keyset in MANY_GROUPS else runs:
        what = "%s, buckets=%s, pred=%s, %d x %d rows" % (keyset, buckets, with_pred, rows // N, N)
        with strides(what) if hashed else contextlib.nullcontext():
            out = run_multi(s, head(b, rows), PRED if with_pred else None, keys, AGGS(s), batch_rows=batch_rows,
                            ref=wide_ref(keyset, with_pred, rows))
        # (a Selection copies raw slots: the filtered batch has no null key)
        assert out is not None and len(out[0]) >= (2 if with_pred else 3)
    assert (_bucketed_batches() > before) == (buckets == "1" and hashed)


@functools.lru_cache(maxsize=None)
def shared_ref(cols):
    s, b = wide_table()
    return oracle_aggregate_grouped_multi(s, head(b, 2 * N), None, [Column(c) for c in cols], AGGS(s), FL, 0)


@pytest.mark.parametrize("buckets", ["0", "1"])
def test_forced_grid_shared_hashes(grid3, buckets):
    """DFMI_GROUP_HASH_BITS=3 on both passes: the rows whose key differs from their slot's are listed from later
    trips (k_group_accumulate) and later tiles (k_group_rank*) and reach the host merge; a Float64 key, a Utf8 key
    and a pair, two batches of N rows."""
    grid3.setenv("DFMI_GROUP_BUCKETS", buckets)
    grid3.setenv("DFMI_GROUP_HASH_BITS", "3")
    s, b = wide_table()
    b = head(b, 2 * N)
    for keys in ([Column(2)], [Column(1)], [Column(0), Column(1)]):
        with strides("3 hash bits, buckets=%s, %d key parts" % (buckets, len(keys))):
            out = run_multi(s, b, None, keys, AGGS(s), batch_rows=N, ref=shared_ref(tuple(k.index for k in keys)))
        assert out is not None and len(out[0]) > 20


# ------------------------------------------ growth and the group-strided passes
@functools.lru_cache(maxsize=None)
def growth_table():
    """The data of test_gpu_agg_batches.test_hash_table_growth_in_one_call -- 40,000 distinct Int64 keys in 64,000
    rows, more than half the first 65,536-slot table -- with a null key: the second row of keys 0..4."""
    rng = np.random.default_rng(805)
    n = 64_000
    perm = rng.permutation(n)
    s = Schema([Field("k", DataType.Int64, True), Field("x", DataType.Float64, False)])
    b = RecordBatch(s, [Array.from_numpy(DataType.Int64, perm % 40_000 * 977, ~((perm >= 40_000) & (perm < 40_005))),
                        Array.from_numpy(DataType.Float64, rng.standard_normal(n))])
    aggs = [agg("SUM", Column(1), s), agg("COUNT", Column(1), s)]
    return s, b, aggs, oracle_aggregate_grouped_multi(s, b, None, [Column(0)], aggs, FL, 0)


@pytest.mark.parametrize("finish", ["device_emit", "host_finish", "norm_rows_0"])
def test_forced_grid_growth_and_group_strided_passes(grid3, finish):
    """40,001 groups from 64,000 rows at three workgroups: the claim overflows the first table and reruns,
    k_group_rehash walks 65,536 slots in trips of 768, k_group_init grows the records. device_emit
    (DFMI_GROUP_DEVICE_EMIT=1): k_group_round, k_group_compact, k_group_sortkey, k_group_nullpos -- the null group
    is there to find -- and k_group_emit over 40,001 groups. host_finish (DFMI_GROUP_HOST_FINISH=1): the records
    read as they stand. norm_rows_0 (DFMI_GROUP_NORM_ROWS=0, two batches): k_group_normalize over groups x float
    SUMs before the second batch."""
    s, b, aggs, ref = growth_table()
    grid3.setenv(*{"device_emit": ("DFMI_GROUP_DEVICE_EMIT", "1"), "host_finish": ("DFMI_GROUP_HOST_FINISH", "1"),
                   "norm_rows_0": ("DFMI_GROUP_NORM_ROWS", "0")}[finish])
    t0 = trips()
    with strides(finish):
        out = run_multi(s, b, None, [Column(0)], aggs, batch_rows=32_000 if finish == "norm_rows_0" else 0, ref=ref)
    assert out is not None and len(out[0]) == 40_001 and out[0][-1][0].is_null
    if finish == "norm_rows_0":
        assert trips() == t0 + 2  # (the first over a table without groups)


# ------------------------------------------------------------ Utf8 MIN / MAX
@functools.lru_cache(maxsize=None)
def string_table() -> Table:
    """Two batches of N rows over ~1,500 Int64 keys (k_sx_init, k_sx_measure and k_sx_keep stride over the groups
    too): test_gpu_minmax_any's random strings over {0x00, a, 0x80, 0xff} (ties past 8 bytes) mixed with its
    hand-built edge strings, 20% nulls."""
    rng = np.random.default_rng(903)
    n = 2 * N
    alpha = np.array([0x00, 0x61, 0x80, 0xff], np.uint8)
    lens, pick, hand = rng.integers(0, 21, n), rng.random(n), rng.integers(0, len(mm.HAND), n)
    strings = [None if p < 0.2 else mm.HAND[h] if p < 0.35 else bytes(alpha[rng.integers(0, 4, int(ln))])
               for ln, p, h in zip(lens, pick, hand)]
    return Table([("k", DataType.Int64, rng.integers(0, 1_500, n) * 1_000_003 - 5_000_000, None),
                  ("s", DataType.Utf8, strings, None)])


@pytest.mark.parametrize("keys", [None, [0]], ids=["ungrouped", "int64"])
def test_forced_grid_utf8_extremes(grid3, keys):
    """MIN(s), MAX(s) at three workgroups, two batches of N rows (the second batch's candidates meet the persisted
    winners): ungrouped -- k_sx_prefix_one -- and over more than 768 groups -- k_sx_prefix, k_sx_candidates over
    the rows, k_sx_init, k_sx_measure and k_sx_keep over the groups."""
    t = string_table()
    with strides("Utf8 extremes, keys=%s" % keys):
        res = mm.srun(t, None, keys, mm.HAGG, batch_rows=N)
    if keys is not None:
        assert len(res[0][0]) > 768
    mm.scheck(t, None, None, keys, mm.HAGG, res)


def test_forced_grid_utf8_arena_compaction(grid3):
    """16 descending batches of 2,000 rows over 1,000 groups, as test_utf8_arena_stays_bounded: every batch
    replaces every group's MIN winner (47 bytes), so the arena fills and k_sx_compact moves the live strings into a
    fresh one -- over 1,000 groups in trips of 768 -- at batches 1, 5 and 14. 94,000 live bytes and 47,000 kept per
    batch fit 2^19 bytes from batch 5 on; without compaction batch 16 would end at 799,000."""
    L = _abi.lib()
    L.dfmi_internal_agg_str_arena_bytes.argtypes = [C.c_void_p]
    L.dfmi_internal_agg_str_arena_bytes.restype = C.c_longlong
    nb, rows, groups = 16, 2_000, 1_000
    n = nb * rows
    s = [b"%06d-%s" % (n - i, b"x" * 40) for i in range(n)]  # descending: each row beats the ones before it
    t = Table([("k", DataType.Int64, np.arange(n) % groups, None), ("s", DataType.Utf8, s, None)])
    aggs = [("MIN", 1), ("MAX", 1)]
    st, cs = mm._state(t, [0], aggs)
    dev = t.batch.to(engine().device)
    reserved = []
    with strides("arena compaction"):
        for b in range(nb):
            st.add(None, slice_batch(dev, b * rows, rows), mm.SFL)
            reserved.append(L.dfmi_internal_agg_str_arena_bytes(st.handle))
    assert reserved[0] == 1 << 18 and reserved[4] == 1 << 19 and reserved[nb - 1] == 1 << 19
    mm.scheck(t, None, None, [0], aggs, mm.collect(t, [0], aggs)(st, cs))


# ------------------------------------------------------------ coalesced entry
# 24 batches of uneven sizes, a 0-row and a 1-row batch among them, N rows in all: 13 past a multiple of 64
COUNTS = [4097, 0, 1, 63, 64, 65, 1000, 1024, 4096, 513, 7, 255, 1999, 2048, 129, 31, 1501, 300, 2, 777, 1201, 640, 90, 654]
assert len(COUNTS) == 24 and sum(COUNTS) == N and N % 64 == 13


@functools.lru_cache(maxsize=None)
def coalesced_table():
    return tb._htable(np.random.default_rng(904), N + 8, 1_000)


COALESCED = {"passed_through": (False, [Column(2), Column(3)]), "evaluated": (True, [Column(2), Column(3)])}


@functools.lru_cache(maxsize=None)
def coalesced_ref(case: str):
    s, b = coalesced_table()
    pred, aggs = tb._hq(s)
    with_pred, keys = COALESCED[case]
    return tb.oracle(s, tb.head(b, N), pred if with_pred else None, keys, aggs)


@pytest.mark.parametrize("device", [True, False], ids=["device_batches", "host_batches"])
def test_forced_grid_coalesced_batches(grid3, device):
    """add_many over the 24 batches at three workgroups == add() batch by batch == the oracle: k_group_concat packs
    the batches' segments dense on later trips -- 8- and 4-byte value jobs and the bit jobs of a Boolean key and of
    validity that is present in some batches only, whose waves own whole destination words by ballot, the last
    wave 13 rows wide -- by an (Int32, Boolean) key pair (one Boolean key alone is the window kernel's), without a
    predicate (the sources are the batches' own columns) and with one (the evaluation pass's segments)."""
    s, b = coalesced_table()
    pred, aggs = tb._hq(s)
    sel = int((b.columns[7].numpy_values()[:N] < 0.8).sum())
    assert sel % 64 != 0 and sel > 768
    for case, (with_pred, keys) in COALESCED.items():
        with strides("coalesced, %s, device=%s" % (case, device)):
            got = tb.check(s, b, COUNTS, pred if with_pred else None, keys, aggs, device=device, ref=coalesced_ref(case))
        assert len(got[0]) >= 3


@functools.lru_cache(maxsize=None)
def narrow_table() -> Table:
    """N rows: Boolean MIN / MAX arguments (`b` with validity in some batches only), a Boolean, an Int8 and an
    Int16 key part, Int32 and Float64 arguments, a predicate column."""
    rng = np.random.default_rng(905)
    vb = rng.random(N) >= 0.15
    vb[2_000:9_000] = True
    return Table([("b", DataType.Boolean, rng.random(N) < 0.9, vb), ("c", DataType.Boolean, rng.random(N) < 0.1, rng.random(N) >= 0.15),
                  ("kb", DataType.Boolean, rng.random(N) < 0.5, rng.random(N) >= 0.05),
                  ("k8", DataType.Int8, rng.integers(-2, 3, N).astype(np.int8), rng.random(N) >= 0.05),
                  ("k16", DataType.Int16, (rng.integers(-20, 20, N) * 1_001).astype(np.int16), None),
                  ("v", DataType.Int32, rng.integers(-2 ** 31, 2 ** 31 - 1, N).astype(np.int32), rng.random(N) >= 0.1),
                  ("x", DataType.Float64, wild_doubles(rng, N), rng.random(N) >= 0.1),
                  ("p", DataType.Float64, rng.random(N), None)])


@pytest.mark.parametrize("host", [False, True], ids=["device_batches", "host_batches"])
def test_forced_grid_coalesced_boolean_extremes(grid3, host):
    """MIN / MAX of Boolean arguments (DFMI_FLAG_EXT_AGG_MINMAX_ANY) through add_many over the 24 batches:
    k_group_bits_to_u8 expands the packed bitmaps (N / 8 bytes: four trips of 768) and k_group_concat runs its 1-,
    2-, 4- and 8-byte and bit jobs on later trips -- (Boolean, Int8, Int16) keys without a predicate, the Int16
    key without nulls with one."""
    t = narrow_table()
    aggs = [("MIN", 0), ("MAX", 0), ("min", 1), ("max", 1), ("SUM", 5), ("SUM", 6), ("COUNT", 0)]
    pred = BinaryExpr(Column(7), Operator.Lt, Literal(Float64(0.6)))
    for p, mask, keys in ((None, None, [2, 3, 4]), (pred, t.values[7] < 0.6, [4])):
        cs = [compile_expr(None, a, t.schema, mm.FL) for a in exprs(t, aggs)]
        st = engine().grouped_agg_state([compile_scalar_expr(None, Column(k), t.schema, mm.FL) for k in keys], cs)
        with strides("Boolean extremes, %d key parts, host=%s" % (len(keys), host)):
            st.add_many(compile_scalar_expr(None, p, t.schema, mm.FL) if p is not None else None,
                        tb.split(t.batch, COUNTS, not host), mm.FL)
            dk, dv = st.finish()
        assert len(dk) >= 40
        mm.check(t, p, mask, keys, aggs, (dk, dv, [None] * len(keys)))


# ------------------------------------------------------- production shape
def test_production_grid_second_and_third_trips(monkeypatch):
    """No grid knob: 2^22 + 3 x 4096 + 77 rows, the schema and data recipe of
    test_group_by_bucketed_accumulation_chosen (1,000 Int64 keys with 1% nulls, nullable wild doubles and Int32,
    the same five aggregates), the oracle evaluated once. The default choice is the bucketed passes (16 buckets x
    128 splits: 4 x 1001 x 128 < n): k_group_rank_fixed and k_group_scatter give blocks 0..2 of the 1,024 a second
    tile, the last of 77 rows, and k_group_claim's 8,192 blocks take a third trip. With DFMI_GROUP_BUCKETS=0
    k_group_accumulate takes the three trips of its real grid."""
    rng = np.random.default_rng(71)
    n = (1 << 22) + 3 * 4096 + 77
    s = Schema([Field("k", DataType.Int64, True), Field("x", DataType.Float64, True), Field("v", DataType.Int32, True)])
    b = RecordBatch(s, [Array.from_numpy(DataType.Int64, rng.integers(0, 1000, n) * 1_000_003, rng.random(n) >= 0.01),
                        Array.from_numpy(DataType.Float64, wild_doubles(rng, n), rng.random(n) >= 0.1),
                        Array.from_numpy(DataType.Int32, rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32),
                                         rng.random(n) >= 0.1)])
    aggs_e = [agg("SUM", Column(1), s), agg("COUNT", Column(1), s), agg("MIN", Column(1), s),
              agg("MAX", Column(2), s), agg("SUM", Column(2), s)]
    ref = oracle_aggregate_grouped_multi(s, b, None, [Column(0)], aggs_e, FL, 0)
    before = _bucketed_batches()
    with strides("production shape, the default choice"):
        out = run_multi(s, b, None, [Column(0)], aggs_e, ref=ref)
    assert out is not None and len(out[0]) == 1001
    assert _bucketed_batches() == before + 1
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_GROUP_BUCKETS", "0")
    with strides("production shape, k_group_accumulate"):
        out = run_multi(s, b, None, [Column(0)], aggs_e, ref=ref)
    assert out is not None and len(out[0]) == 1001
    assert _bucketed_batches() == before + 1
