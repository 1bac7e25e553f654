"""Aggregate relation (DFMI_FLAG_EXT_AGGREGATE): LogicalPlan::Aggregate over
an optional Selection (sqlplanner.rs:91-117), without or with one GROUP BY
key. The reference plans it and compiles its AggregateFunctions (compile_expr,
expression.rs:81-116) but its executor stops at context.rs:161
(`unimplemented!()`); here every input batch is one fused predicate +
aggregate pass on the GPU and next() returns the result: one row, or one row
per group in key order (null key last)."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from ..arrow import Array, RecordBatch, Schema
from ..logicalplan import DataType
from .engine import engine
from .filter import detach
from .relation import Relation

_NP = {
    DataType.Int8: np.int8, DataType.Int16: np.int16, DataType.Int32: np.int32, DataType.Int64: np.int64,
    DataType.UInt8: np.uint8, DataType.UInt16: np.uint16, DataType.UInt32: np.uint32, DataType.UInt64: np.uint64,
    DataType.Float32: np.float32, DataType.Float64: np.float64,
}


def agg_value_array(v) -> Array:
    """A one-row Array holding an aggregate value (dfmi_agg_value)."""
    t = DataType(v.type)
    if t == DataType.Boolean:  # MIN / MAX of a Boolean argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY)
        return Array.from_numpy(t, np.array([bool(v.bits)]), np.array([False]) if v.is_null else None)
    dt = np.dtype(_NP[t])
    raw = np.array([v.bits], dtype=np.uint64).view(np.uint8)[: dt.itemsize].copy()
    vals = raw.view(dt)
    return Array.from_numpy(t, vals, np.array([not v.is_null]) if v.is_null else None)


def agg_values_array(vals) -> Array:
    """An Array of several aggregate / group-key values (dfmi_agg_value), one
    row each: a list of them, or a one-dimensional record array over their
    layout (a finish's column: no Python loop over the groups)."""
    if isinstance(vals, np.ndarray):
        if len(vals) == 0:
            return Array.from_pylist(DataType.Boolean, [])
        t = DataType(int(vals["type"][0]))
        valid = vals["is_null"] == 0
        bits = np.ascontiguousarray(vals["bits"])
        if t == DataType.Boolean:
            return Array.from_numpy(t, bits != 0, None if valid.all() else valid)
        dt = np.dtype(_NP[t])
        raw = bits.view(np.uint8).reshape(-1, 8)[:, : dt.itemsize].copy()
        return Array.from_numpy(t, raw.reshape(-1).view(dt), None if valid.all() else valid)
    if not vals:
        return Array.from_pylist(DataType.Boolean, [])
    t = DataType(vals[0].type)
    valid = np.array([not v.is_null for v in vals])
    if t == DataType.Boolean:
        return Array.from_numpy(t, np.array([bool(v.bits) for v in vals]), None if valid.all() else valid)
    dt = np.dtype(_NP[t])
    raw = np.array([v.bits for v in vals], dtype=np.uint64).view(np.uint8).reshape(-1, 8)[:, : dt.itemsize].copy()
    return Array.from_numpy(t, raw.reshape(-1).view(dt), None if valid.all() else valid)


def agg_value_py(v):
    """The aggregate value as a Python scalar (None for null)."""
    if v.is_null:
        return None
    return agg_value_array(v).numpy_values()[0].item()


class AggregateRelation(Relation):
    """Aggregate(input, group_expr, aggr_expr) with the input's Selection (if
    any) fused: pulls every batch of `input`, then yields one batch -- the
    group key columns (if any, in group_expr order) followed by the
    aggregates, one row per group in key order. With coalesce > 1, up to that
    many input batches (at most 2^20 rows) are read ahead and accumulated by
    one call (AggState.add_many) while the next group is read; the result and
    the first error are those of one call per pull."""

    def __init__(self, input: Relation, predicate, aggs: List, schema: Schema, device=None, flags: int = 0,
                 key=None, coalesce: int = 1):
        self.input = input
        self.predicate = predicate
        self.aggs = aggs
        # one RuntimeExpr (the single-key form) or a list of them
        self.keys = None if key is None else (list(key) if isinstance(key, (list, tuple)) else [key])
        self._schema = schema
        self.device = device
        self.flags = flags
        self.coalesce = coalesce
        self.done = False

    def _read_ahead(self, m: int, max_rows: int = 1 << 20):
        """Up to m batches / max_rows rows of the input, and the error the
        input raised after them (None otherwise), as Coalescer._read_ahead."""
        many = getattr(self.input, "next_many", None)
        if many is not None:
            try:
                return many(m, max_rows), None
            except Exception as e:
                return [], e
        pulled, rows = [], 0
        while len(pulled) < m and rows < max_rows:
            try:
                b = self.input.next()
            except Exception as e:  # raised after the batches before it
                return pulled, e
            if b is None:
                break
            if b._transient:
                b = detach(b)
            pulled.append(b)
            rows += b.num_rows()
        return pulled, None

    def _add_coalesced(self, eng, state) -> None:
        """The pull loop in groups of up to `coalesce` batches, each one
        add_many call on the engine's worker thread while the next group is
        read; errors in the order one pull per batch would have raised them."""
        from concurrent.futures import ThreadPoolExecutor
        if eng._worker is None:
            eng._worker = ThreadPoolExecutor(max_workers=1, thread_name_prefix="dfmi-engine")
        stream = eng.current_stream()  # (this thread's: the worker would see its own)
        inflight = None
        while True:
            pulled, src_err = self._read_ahead(self.coalesce)
            if inflight is not None:
                inflight.result()  # (an earlier group's error comes first)
                inflight = None
            if pulled:
                eng.drain()
                inflight = eng._worker.submit(state._add_runs, self.predicate, pulled, self.flags, stream)
                eng._inflight = inflight  # (every other entry point waits for it first)
            if src_err is not None or not pulled:
                if inflight is not None:
                    inflight.result()
                if src_err is not None:
                    raise src_err
                return

    def next(self) -> Optional[RecordBatch]:
        if self.done:
            return None
        self.done = True
        eng = engine(self.device)
        state = eng.agg_state(self.aggs) if self.keys is None else eng.grouped_agg_state(self.keys, self.aggs)
        if self.coalesce > 1:
            self._add_coalesced(eng, state)
        else:
            while True:
                b = self.input.next()
                if b is None:
                    break
                state.add(self.predicate, b, self.flags)
        if self.keys is None:  # (a Utf8 MIN / MAX: its bytes from the state, None for null)
            return RecordBatch(self._schema, [Array.from_strings(state.value_strings(j)) if DataType(v.type) == DataType.Utf8
                                              else agg_value_array(v) for j, v in enumerate(state.finish())])
        keys, vals = state.finish()
        if len(keys) == 0:
            return None
        nk = len(self.keys)
        cols = []
        for p in range(nk):  # (the state is created with the key list: keys[group][part])
            kv = keys[:, p]
            if DataType(int(kv["type"][0])) == DataType.Utf8:
                cols.append(Array.from_strings(state.key_strings(p)))
            else:
                cols.append(agg_values_array(kv))
        for j in range(len(self.aggs)):
            if DataType(int(vals[0, j]["type"])) == DataType.Utf8:
                cols.append(Array.from_strings(state.value_strings(j)))
            else:
                cols.append(agg_values_array(vals[:, j]))
        return RecordBatch(self._schema, cols)

    def schema(self) -> Schema:
        return self._schema
