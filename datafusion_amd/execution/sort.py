"""Sort and Limit relations (DFMI_FLAG_EXT_SORT): LogicalPlan::Sort and
LogicalPlan::Limit (sqlplanner.rs:119-163), which the reference plans and its
executor leaves at context.rs:161 (`unimplemented!()`).

SortRelation is a pipeline breaker: it pulls every batch of its input onto the
GPU, orders all rows with one dfmi_sort_batches call (stable, DESIGN.md §2
order, optionally only the first `limit` rows) and returns one batch.
LimitRelation streams: it hands input batches on and cuts the last one."""
from __future__ import annotations

from typing import List, Optional, Sequence

from ..arrow import RecordBatch, Schema
from ..logicalplan import Column, Expr, SortExpr
from .engine import engine
from .error import ExecutionError
from .expression import compile_scalar_expr
from .relation import Relation

MAX_SORT_KEYS = 8  # csrc/sort.h kMaxKeys


class SortRelation(Relation):
    """Sort(input, keys) [+ Limit]: `keys` are SortExprs (or bare expressions,
    ascending) over the input schema. A key that is a plain Column sorts by
    that input column; any other is evaluated over each input batch by the
    fused projection (the input columns plus the key expressions), so its
    runtime errors are the projection's, and dropped from the result."""

    def __init__(self, input: Relation, keys: Sequence[Expr], schema: Schema, device=None, flags: int = 0,
                 limit: Optional[int] = None, ctx=None):
        if len(keys) > MAX_SORT_KEYS:
            raise ExecutionError("NotImplemented", "device program limit: more than %d ORDER BY expressions"
                                 % MAX_SORT_KEYS)
        self.input = input
        self._schema = schema
        self.device = device
        self.flags = flags
        self.limit = limit
        self.done = False
        ncols = len(schema)
        self.key_columns: List[int] = []
        self.key_asc: List[bool] = []
        helpers = []
        for k in keys:
            e, asc = (k.expr, k.asc) if isinstance(k, SortExpr) else (k, True)
            if isinstance(e, Column):
                if not 0 <= e.index < ncols:
                    raise ExecutionError("InvalidColumn", "ORDER BY column #%d" % e.index)
                self.key_columns.append(e.index)
            else:
                self.key_columns.append(ncols + len(helpers))
                helpers.append(e)
            self.key_asc.append(bool(asc))
        # input columns passed through + the key expressions, one fused pass per batch
        self._projs = None
        if helpers:
            self._projs = [compile_scalar_expr(ctx, e, schema, flags) for e in [Column(i) for i in range(ncols)] + helpers]

    def next(self) -> Optional[RecordBatch]:
        if self.done:
            return None
        self.done = True
        if self.limit == 0:
            return None
        eng = engine(self.device)
        batches = []
        while True:
            b = self.input.next()
            if b is None:
                break
            if b.num_rows() == 0:
                continue
            b = eng.to_device(b)  # (a copy of a host batch: a source's transient view may be overwritten)
            if self._projs is not None:
                b = RecordBatch(b.schema, eng.filter_project(None, self._projs, b, self.flags))
            batches.append(b)
        if not batches:
            return None
        cols = eng.sort_batches(batches, self.key_columns, self.key_asc, self.limit, self.flags)
        return RecordBatch(self._schema, cols[:len(self._schema)])

    def schema(self) -> Schema:
        return self._schema


class LimitRelation(Relation):
    """Limit(input, n): the first n rows of the input in its order."""

    def __init__(self, input: Relation, limit: int, schema: Schema = None):
        self.input = input
        self.remaining = int(limit)
        self._schema = schema if schema is not None else input.schema()

    def next(self) -> Optional[RecordBatch]:
        if self.remaining <= 0:
            return None
        b = self.input.next()
        if b is None:
            return None
        rows = b.num_rows()
        if rows <= self.remaining:
            self.remaining -= rows
            return b
        out = RecordBatch(b.schema, [c.slice(0, self.remaining) for c in b.columns])
        out._transient = b._transient
        self.remaining = 0
        return out

    def schema(self) -> Schema:
        return self._schema
