"""CSV output (DFMI_FLAG_EXT_CSV_WRITE): PhysicalPlan::Write { plan, filename,
kind: "csv" } (physicalplan.rs:24-29), which the reference defines and never
runs. The records are encoded on the device (dfmi_csv_encode_batches, all the
batches of a group in one call), copied to pinned host memory and appended to
the file; the dialect -- what CsvDataSource / NativeCsvDataSource read back to
the same values -- is specified at the flag in include/dfmi.h."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from .. import _abi
from ..arrow import RecordBatch, Schema
from .engine import engine
from .error import ExecutionError

MAX_GROUP_ROWS = 1 << 20  # rows per encode call, as the relations' read-ahead (filter.py Coalescer)
_BYTE_LIMIT = "device program limit: CSV output of 2^31 or more bytes"


def csv_header(schema: Schema) -> bytes:
    """The header line of `schema` (dfmi_csv_header: host only, no context)."""
    L = _abi.lib()
    sch, keep = _abi.make_schema([(f.name, f.data_type, f.nullable) for f in schema.fields])
    n = C.c_int64(0)
    err = _abi.dfmi_error()
    rc = L.dfmi_csv_header(C.byref(sch), None, 0, C.byref(n), C.byref(err))
    if rc == _abi.DFMI_OK:
        buf = (C.c_uint8 * max(1, n.value))()
        rc = L.dfmi_csv_header(C.byref(sch), buf, n.value, C.byref(n), C.byref(err))
    if rc != _abi.DFMI_OK:
        raise ExecutionError.from_status(rc, err.message.decode("utf-8", errors="replace"))
    return bytes(buf[:n.value])


class CsvWriter:
    """A CSV file of `schema`: the header on creation, then whole records per
    write(). Host batches are uploaded first (eng.to_device)."""

    def __init__(self, path: str, schema: Schema, has_header: bool = True, device=None,
                 flags: int = _abi.DFMI_FLAG_EXT_CSV_WRITE):
        self.schema = schema
        self.device = device
        self.flags = flags
        self.rows = 0
        self._pinned = None
        header = csv_header(schema) if has_header else b""  # (before the file exists: a bad schema leaves none)
        self._file = open(path, "wb")
        self._file.write(header)

    def write(self, batches: Sequence[RecordBatch]) -> int:
        """Appends the batches' records (one encode call; a group whose bytes
        reach 2^31 is halved). Returns the rows written."""
        batches = [b for b in batches]
        if not batches:
            return 0
        eng = engine(self.device)
        try:
            data, _ = eng.csv_encode_batches(batches, self.flags)
        except ExecutionError as e:
            if len(batches) > 1 and e.kind == "NotImplemented" and e.message == _BYTE_LIMIT:
                half = len(batches) // 2
                return self.write(batches[:half]) + self.write(batches[half:])
            raise
        n = data.numel()
        if n:
            if self._pinned is None or self._pinned.numel() < n:
                self._pinned = torch.empty(max(n, 1 << 16), dtype=torch.uint8, pin_memory=True)
            host = self._pinned[:n]
            host.copy_(data, non_blocking=True)
            torch.cuda.current_stream(eng.device).synchronize()
            self._file.write(memoryview(host.numpy()))
        rows = sum(b.num_rows() for b in batches)
        self.rows += rows
        return rows

    def close(self) -> None:
        if self._file is not None:
            self._file.close()
            self._file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_relation(rel, path: str, has_header: bool = True, device=None, flags: int = _abi.DFMI_FLAG_EXT_CSV_WRITE,
                   coalesce: int = 256) -> int:
    """Pulls `rel` dry into the CSV file `path`: up to `coalesce` batches or
    2^20 rows per encode call. An error from a pull or an encode propagates as
    it is; the file then holds the header and the whole records of the batches
    before it."""
    eng = engine(device)
    rows = 0
    with CsvWriter(path, rel.schema(), has_header, device, flags) as w:
        done = False
        while not done:
            group, n, error = [], 0, None
            while len(group) < max(1, coalesce) and n < MAX_GROUP_ROWS:
                try:
                    b = rel.next()
                except ExecutionError as e:
                    error = e  # (after the batches pulled before it, as a pull loop would have seen it)
                    break
                if b is None:
                    done = True
                    break
                group.append(eng.to_device(b))  # (a copy of a host batch: a source's transient view may be overwritten)
                n += b.num_rows()
            rows += w.write(group)
            if error is not None:
                raise error
    return rows
