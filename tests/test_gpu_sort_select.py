"""Sort / Limit on the device past one select tile and past one grid of
workgroups, against the restatements of tests/test_gpu_sort.py (never the
device against itself, every column bit for bit through its check()).

Multi-tile select: 3 x 4096 + 17 rows -- three full tiles of the top-k
prefilter and a ragged one, so the scanned tile bases are non-zero -- with the
prefilter forced on and dfmi_internal_sort_select proving that it ran and how
many rows it kept. Reference: expected_order (Python's stable sorted).

Loops past one grid, no switches: 1,026 select tiles (k_sort_hist,
k_sort_count and k_sort_select stride past their 1,024 workgroups), 600,011
rows (k_sort_gather_bits, k_sort_utf8_max and k_sort_utf8_len stride past
524,288 rows), and the full-sort key types at 100,003 rows. Reference:
expected_order_np, which tests/test_sort_cpu.py pins to expected_order.

Not reached: k_sort_word, k_sort_gather and k_sort_utf8_copy stride only past
65,536 workgroups x 256 rows (or x 4 waves x 64 rows) = 16.7M rows, which no
test that takes seconds can build and check on the host."""
import ctypes as C
import functools

import numpy as np
import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import RecordBatch, np_dtype
from datafusion_amd.execution.engine import engine
from datafusion_amd.logicalplan import DataType
from test_gpu_sort import (F32_SPECIAL, Col, batches_of, check, column, entropy, expected_order,
                           expected_order_np, run, sizes_for)

pytestmark = pytest.mark.gpu

T = DataType
TILE = 4096  # csrc/sort.h kSelectRows
N = 3 * TILE + 17


def select_info():
    """(did the last sort on the engine's context run the prefilter, rows it handed to the radix passes)"""
    f = _abi.lib().dfmi_internal_sort_select
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    f.restype = C.c_int32
    out = (C.c_uint64 * 2)()
    assert f(engine("cuda:0").ctx, out) == _abi.DFMI_OK
    return int(out[0]), int(out[1])


def uniform(t, n, rng, nulls=True):
    """An integer column uniform over the type's whole range, the extremes among it."""
    ii = np.iinfo(np_dtype(t))
    vals = rng.integers(ii.min, ii.max, n, dtype=ii.dtype, endpoint=True)
    vals[:4] = [ii.min, ii.max, ii.max - 1, ii.min + 1]
    return Col(t, rng.permutation(vals), rng.random(n) >= 0.2 if nulls else None)


def ints(vals, rng, nulls):
    return Col(T.Int64, vals, rng.random(len(vals)) >= 0.1 if nulls else None)


# ---- multi-tile select, prefilter forced on
# name -> (columns, keys of the ASC run (the DESC run reverses every key), what the hook's row count must show,
# input batches or None for sizes_for(n, True)). The row count: "small", fewer than n rows for limits <= 7;
# "small cut", also for the limit inside the first tie group; "all", n rows whatever the limit.
@functools.lru_cache(maxsize=None)
def select_case(name):
    rng = np.random.default_rng(sorted(SELECT_CASES).index(name) + 61)
    n = N
    idx = Col(T.Int32, np.arange(n))
    r300 = rng.integers(0, 300, n).astype(np.int64)
    if name in ("f64_entropy", "i64_entropy", "u64_entropy"):
        key = entropy({"f": T.Float64, "i": T.Int64, "u": T.UInt64}[name[0]], n, rng)
        if name[0] == "u":  # a valid 2^64 - 1 beside the nulls: the same word
            assert (key.vals[key.valid] == np.uint64(2**64 - 1)).any() and not key.valid.all()
        if name[0] == "f":
            nan = np.isnan(key.vals) & key.valid
            assert (nan & np.signbit(key.vals)).any() and (nan & ~np.signbit(key.vals)).any()
        return [key, idx], [(0, True)], "small", None
    if name.startswith("i64_last_pass"):  # five passes see one digit, the 9-bit bottom pass decides
        return [ints((1 << 40) + r300, rng, name.endswith("nulls")), idx], [(0, True)], "", None
    if name.startswith("i64_first_pass"):  # the top 11 bits decide, every pass below sees one digit
        return [ints(r300 << 53, rng, name.endswith("nulls")), idx], [(0, True)], "", None
    if name.startswith("i64_three_values"):  # tie groups of ~4,100 rows (~3,700 with nulls) over every tile
        vals = np.array([-5, 1 << 40, 7], dtype=np.int64)[rng.integers(0, 3, n)]
        return [ints(vals, rng, name.endswith("nulls")), idx], [(0, True)], "small cut", None
    if name == "i8_nulls":
        return [column(T.Int8, n, rng, True), idx], [(0, True)], "", None
    if name == "bool_nulls":
        return [column(T.Boolean, n, rng, True), idx], [(0, True)], "", None
    if name in ("i32_nulls", "u32_nulls"):
        return [uniform(T.Int32 if name[0] == "i" else T.UInt32, n, rng), idx], [(0, True)], "", None
    if name == "f32_nulls":
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        vals[:len(F32_SPECIAL)] = F32_SPECIAL.view(np.uint32)
        return [Col(T.Float32, rng.permutation(vals).view(np.float32), rng.random(n) >= 0.2), idx], [(0, True)], "", None
    if name == "utf8_lead":  # STRINGS: short, trailing \0, equal first chunks, \xff-leading, 300 bytes
        return [column(T.Utf8, n, rng, True), idx], [(0, True)], "", None
    if name == "all_words_equal":
        return ([Col(T.Int64, np.full(n, 42)), column(T.Int16, n, rng, True), idx], [(0, True), (1, False)], "all", None)
    assert name == "sliced_f64"
    n, off = 12500, 13
    cols = [column(T.Float64, n, rng, True), Col(T.Int32, np.arange(n))]
    whole = batches_of(cols, [n])[0]
    cut = [(off, 5000), (3, 0), (off + 5000 + 5, 3750), (1, 175)]  # test_sliced_input's cuts x 25: 8,925 rows
    batches = [RecordBatch(whole.schema, [a.slice(o, ln) for a in whole.columns]) for o, ln in cut]
    rows = [i for o, ln in cut for i in range(o, o + ln)]
    assert len(rows) > 2 * TILE
    return [c.take(rows) for c in cols], [(0, True)], "", tuple(batches)


SELECT_CASES = ["f64_entropy", "i64_entropy", "u64_entropy", "i64_last_pass", "i64_last_pass_nulls", "i64_first_pass",
                "i64_first_pass_nulls", "i64_three_values", "i64_three_values_nulls", "i8_nulls", "bool_nulls",
                "i32_nulls", "u32_nulls", "f32_nulls", "utf8_lead", "all_words_equal", "sliced_f64"]


def tie_cut(lead, full):
    """A limit inside the first group of rows tied on the leading key that reaches past row 7, or None."""
    from test_gpu_sort import comparable
    vals = comparable(lead)
    start = 0
    for p in range(1, len(full) + 1):
        if p == len(full) or vals[full[p]] != vals[full[start]]:
            if p - start >= 2 and start + (p - start) // 2 > 7:
                return start + (p - start) // 2
            start = p
    return None


@pytest.mark.parametrize("asc", [True, False], ids=["asc", "desc"])
@pytest.mark.parametrize("name", SELECT_CASES)
def test_select_over_several_tiles(name, asc, monkeypatch):
    cols, keys, expect, batches = select_case(name)
    if not asc:
        keys = [(j, not a) for j, a in keys]
    n = cols[0].n
    if batches is None:
        batches = batches_of(cols, sizes_for(n, True))
    batches = [b.to("cuda:0") for b in batches]
    full = expected_order(cols, keys)
    cut = tie_cut(cols[keys[0][0]], full)
    nonnull = int(cols[keys[0][0]].valid.sum())
    assert cut is not None  # (every case has nulls or repeated values in its leading key)
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_SORT_SELECT", "1")
    # nonnull + 3: the k-th word is a null's; where the leading key has no null that is past n, and no select
    for limit in [k for k in (1, 7, cut, nonnull + 3, n - 1) if k < n]:
        out = run(cols, keys, limit=limit, batches=batches)
        ran, kept = select_info()
        print("%s %s limit %d: select %d, %d of %d rows kept" % (name, "asc" if asc else "desc", limit, ran, kept, n))
        assert ran == 1
        assert limit <= kept <= n
        if ("small" in expect and limit <= 7) or ("cut" in expect and limit == cut):
            assert kept < n
        if expect == "all":
            assert kept == n
        check(out, cols, full[:limit])


def test_without_the_prefilter_the_hook_says_so(monkeypatch):
    cols, keys, _, _ = select_case("i64_entropy")
    monkeypatch.setenv("DFMI_DIAG", "1")
    monkeypatch.setenv("DFMI_SORT_SELECT", "0")
    run(cols, keys, limit=7)
    assert select_info() == (0, cols[0].n)
    monkeypatch.setenv("DFMI_SORT_SELECT", "1")
    run(cols, keys)  # no limit: nothing to select
    assert select_info() == (0, cols[0].n)


# ---- loops past one grid, defaults only
@functools.lru_cache(maxsize=None)
def stride_table():
    """1,026 select tiles: tie groups of a nullable Int64 in [-500, 500) that span more than a thousand tiles each."""
    n = 1025 * TILE + 5
    rng = np.random.default_rng(71)
    cols = [Col(T.Int64, rng.integers(-500, 500, n), rng.random(n) >= 0.1), Col(T.Int64, np.arange(n)),
            Col(T.Boolean, rng.random(n) < 0.5, rng.random(n) >= 0.3)]
    sizes = [1_500_001, 2_000_000, n - 3_500_001]
    return cols, [b.to("cuda:0") for b in batches_of(cols, sizes)]


@pytest.mark.parametrize("asc", [True, False], ids=["asc", "desc"])
def test_select_strides_past_its_grid(asc, monkeypatch):
    monkeypatch.delenv("DFMI_SORT_SELECT", raising=False)
    cols, batches = stride_table()
    n = cols[0].n
    assert (n + TILE - 1) // TILE > 1024
    keys = [(0, asc)]
    full = expected_order_np(cols, keys)
    # n // 8: the default switch ratio's edge, and an output bitmap of 8,200 words (k_sort_gather_bits' waves cover 8,192)
    for limit in (1000, n // 8):
        out = run(cols, keys, limit=limit, batches=batches)
        ran, kept = select_info()
        print("stride %s limit %d: select %d, %d of %d rows kept" % ("asc" if asc else "desc", limit, ran, kept, n))
        assert ran == 1 and limit <= kept < n
        check(out, cols, full[:limit])


@functools.lru_cache(maxsize=None)
def gather_table():
    """600,011 rows: past the 524,288 that k_sort_gather_bits, k_sort_utf8_max and k_sort_utf8_len cover at once."""
    n = 600_011
    rng = np.random.default_rng(72)
    pool = [bytes(rng.integers(32, 127, ln, dtype=np.uint8)) for ln in rng.integers(0, 41, 400)]  # 0-40 bytes
    pool += [b"", b"sameprfx", b"sameprfxA", b"sameprfx\0", b"sixteen-byte-pre", b"sixteen-byte-preX"]
    assert sum(len(s) > 16 for s in pool) > 3  # (csrc/sort.h kShortString)
    pick = lambda: [pool[i] for i in rng.integers(0, len(pool), n)]
    cols = [Col(T.Utf8, pick(), rng.random(n) >= 0.2), Col(T.Boolean, rng.random(n) < 0.5, rng.random(n) >= 0.3),
            Col(T.Utf8, pick(), rng.random(n) >= 0.3), Col(T.Int32, np.arange(n)),
            Col(T.Int64, rng.integers(-(1 << 62), 1 << 62, n), rng.random(n) >= 0.2)]
    return cols, [b.to("cuda:0") for b in batches_of(cols, [250_001, 0, 349_999, 11])]


@pytest.mark.parametrize("keys", [[(0, True)], [(4, False)]], ids=["utf8_asc", "i64_desc"])
def test_gather_and_utf8_stride_past_their_grids(keys):
    cols, batches = gather_table()
    assert cols[0].n > 2048 * 256
    out = run(cols, keys, batches=batches)
    assert select_info() == (0, cols[0].n)
    check(out, cols, expected_order_np(cols, keys))


@functools.lru_cache(maxsize=None)
def many_blocks_table():
    n = 100_003
    rng = np.random.default_rng(73)
    cols = [entropy(T.Float64, n, rng), column(T.Utf8, n, rng, True), Col(T.Int64, rng.integers(-3, 3, n), rng.random(n) >= 0.2),
            Col(T.Int32, np.arange(n))]
    return cols, [b.to("cuda:0") for b in batches_of(cols, sizes_for(n, True))]


@pytest.mark.parametrize("keys", [[(0, True)], [(1, True)], [(1, False), (2, True)]], ids=["f64", "utf8", "utf8_desc_i64"])
def test_full_sort_keys_over_many_blocks(keys):
    cols, batches = many_blocks_table()
    check(run(cols, keys, batches=batches), cols, expected_order_np(cols, keys))
