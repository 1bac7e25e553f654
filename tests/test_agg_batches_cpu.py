"""Coalesced aggregate (dfmi_aggregate_batches / dfmi_aggregate_host_batches)
without a device: the batched form of the aggregate kernels generates and
compiles with hipRTC for gfx950, the entry points are exported and declared,
and AggregateRelation's read-ahead keeps the pull loop's error order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from datafusion_amd import _abi
from datafusion_amd.arrow import Array, Field, RecordBatch, Schema
from datafusion_amd.execution.aggregate import AggregateRelation
from datafusion_amd.execution.error import ExecutionError
from datafusion_amd.logicalplan import BinaryExpr, Column, DataType, Float64, Literal, Operator
from test_aggregate_cpu import AGG, _agg_jit, _grouped_jit, agg

BATCHED = 0x40000000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schema():
    return Schema([Field("k", DataType.Int32, True), Field("x", DataType.Float64, True),
                   Field("i", DataType.Int32, False), Field("b", DataType.Boolean, True)])


def _queries(s):
    pred = BinaryExpr(Column(1), Operator.Lt, Literal(Float64(0.7)))
    aggs = [agg("SUM", Column(1), s), agg("MIN", Column(2), s), agg("COUNT", Column(1), s), agg("MAX", Column(1), s)]
    return pred, aggs


@pytest.mark.parametrize("with_pred", [False, True])
def test_batched_ungrouped_kernel_compiles(with_pred):
    s = _schema()
    pred, aggs = _queries(s)
    p = pred if with_pred else None
    flags = AGG | _abi.DFMI_FLAG_EXT_GATHER_ALL
    rc, code, msg, src = _agg_jit(s, p, aggs, flags | BATCHED)
    assert rc > 0, msg
    body = src[src.index("generated query kernel"):]
    # a block finds its batch, its rows and its own error word in the table; the accumulators stay the call's
    assert "A0.tile_batch[bid_]" in body and "A.err = (u64*)bp_[3]" in body and "A.n_rows = (i64)(u64)bp_[0]" in body
    assert "A.valid[0] = (const u8*)bp_[" in body  # the nullable argument's validity per batch
    assert "A.agg =" not in body and "A.status" not in body
    assert "atomicAdd(A.totals" not in body  # no selectivity hint from the coalesced form
    # the one-batch form is what it was
    rc1, _, msg1, src1 = _agg_jit(s, p, aggs, flags, compile_=False)
    assert rc1 > 0, msg1
    body1 = src1[src1.index("generated query kernel"):]
    assert "tile_batch" not in body1 and "const dfmi::Args& A = A0;" in body1
    assert ("atomicAdd(A.totals" in body1) == with_pred
    # ... and the batched form is that body behind the prologue
    tail = body1[body1.index("constexpr int NA"):]
    tail = "\n".join(l for l in tail.split("\n") if "atomicAdd(A.totals" not in l)
    assert body[body.index("constexpr int NA"):] == tail


@pytest.mark.parametrize("key", [0, 3])
@pytest.mark.parametrize("with_pred", [False, True])
def test_batched_grouped_kernel_compiles(key, with_pred):
    s = _schema()
    pred, aggs = _queries(s)
    p = pred if with_pred else None
    rc, code, msg, src = _grouped_jit(s, p, Column(key), aggs, AGG | _abi.DFMI_FLAG_EXT_GATHER_ALL | BATCHED)
    assert rc > 0, msg
    body = src[src.index("generated query kernel"):]
    assert "A0.tile_batch[bid_]" in body and "gsl[k]" in body and "GS = %d" % (17 if key == 0 else 3) in body
    rc1, _, msg1, src1 = _grouped_jit(s, p, Column(key), aggs, AGG | _abi.DFMI_FLAG_EXT_GATHER_ALL, compile_=False)
    assert rc1 > 0, msg1
    body1 = src1[src1.index("generated query kernel"):]
    assert "tile_batch" not in body1
    assert body[body.index("constexpr int NA"):] == body1[body1.index("constexpr int NA"):]


def test_entry_points_exported_and_declared():
    L = _abi.lib()
    hdr = open(os.path.join(ROOT, "include", "dfmi.h")).read()
    for name in ("dfmi_aggregate_batches", "dfmi_aggregate_host_batches"):
        assert name in _abi.EXPORTED
        assert getattr(L, name).argtypes is not None
        assert re.search(r"\b%s\(" % name, hdr)
    assert _abi.DFMI_ABI_VERSION == 4
    hook = L.dfmi_internal_agg_query_launches
    hook.restype = C.c_long
    assert hook() >= 0
    assert "dfmi_internal_agg_query_launches" not in hdr
    # num_batches == 0 is a no-op that needs no device; NULL arguments are rejected
    err = _abi.dfmi_error()
    failed = C.c_int32(7)
    assert L.dfmi_aggregate_batches(None, None, None, None, 0, AGG, C.byref(failed), C.byref(err)) != _abi.DFMI_OK
    assert failed.value == -1 and err.message.decode() == "NULL argument"


# ---- AggregateRelation's read-ahead, with a stub engine and state

class _Eng:
    def __init__(self):
        self._worker = None
        self._inflight = None

    def current_stream(self):
        return 0

    def drain(self):
        f, self._inflight = self._inflight, None
        if f is not None:
            from concurrent.futures import wait
            wait([f])


class _State:
    def __init__(self, fail_at=None):
        self.seen, self.calls, self.fail_at = [], [], fail_at

    def _add_runs(self, predicate, batches, flags=0, stream=None):
        self.calls.append(len(batches))
        for b in batches:
            if self.fail_at is not None and len(self.seen) == self.fail_at:
                raise ExecutionError("General", "batch %d failed" % self.fail_at)
            self.seen.append(b.num_rows())


class _Source:
    """Batch i has i + 1 rows; pull `raise_at` raises."""

    def __init__(self, n, raise_at=None):
        self.s = Schema([Field("x", DataType.Float64, False)])
        self.n, self.i, self.raise_at = n, 0, raise_at

    def next(self):
        if self.raise_at is not None and self.i == self.raise_at:
            self.i += 1
            raise ExecutionError("General", "source failed")
        if self.i >= self.n:
            return None
        self.i += 1
        return RecordBatch(self.s, [Array.from_numpy(DataType.Float64, np.zeros(self.i))])

    def schema(self):
        return self.s


def _pull(src, state, coalesce):
    rel = AggregateRelation(src, None, [], src.schema(), coalesce=coalesce)
    eng = _Eng()
    try:
        rel._add_coalesced(eng, state)
    finally:
        if eng._worker is not None:
            eng._worker.shutdown()


@pytest.mark.parametrize("coalesce", [2, 3, 7, 256])
def test_read_ahead_groups_in_order(coalesce):
    st = _State()
    _pull(_Source(10), st, coalesce)
    assert st.seen == list(range(1, 11))
    assert st.calls == [min(coalesce, 10 - i) for i in range(0, 10, coalesce)]


@pytest.mark.parametrize("coalesce", [2, 4, 256])
@pytest.mark.parametrize("j", [0, 3, 5])
def test_source_error_after_the_batches_before_it(coalesce, j):
    st = _State()
    with pytest.raises(ExecutionError) as ei:
        _pull(_Source(10, raise_at=j), st, coalesce)
    assert ei.value.message == "source failed"
    assert st.seen == list(range(1, j + 1))  # add_many saw batches [0, j) first


@pytest.mark.parametrize("coalesce", [2, 4, 256])
def test_add_many_error_wins_over_later_source_error(coalesce):
    st = _State(fail_at=2)
    with pytest.raises(ExecutionError) as ei:
        _pull(_Source(10, raise_at=5), st, coalesce)
    assert ei.value.message == "batch 2 failed"
    assert st.seen == [1, 2]
