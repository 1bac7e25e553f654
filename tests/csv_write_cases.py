"""CSV output (DFMI_FLAG_EXT_CSV_WRITE): what the CPU and the GPU tests share.

`encode_batches` is the Python restatement of the contract in include/dfmi.h --
numbers through logicalplan.rust_float / str(int), the quoting rule written
out directly -- and the only source of expected bytes: nothing here comes from
the device, and Python's csv.writer is not used (with lineterminator="\\n" it
leaves a field holding "\\r" unquoted). `assert_reads_back` is the round-trip
rule: valid slots bit for bit, NaN as the canonical quiet NaN, equal null
counts, a Utf8 null as ""."""
import numpy as np

from datafusion_amd.arrow import Array, Field, RecordBatch, Schema, np_dtype
from datafusion_amd.logicalplan import DataType, rust_float

BOOL, F32, F64, UTF8 = DataType.Boolean, DataType.Float32, DataType.Float64, DataType.Utf8
INTS = [DataType.Int8, DataType.Int16, DataType.Int32, DataType.Int64, DataType.UInt8, DataType.UInt16,
        DataType.UInt32, DataType.UInt64]
TYPES = [BOOL] + INTS + [F32, F64, UTF8]
SPECIAL = b'",\n\r'


# ------------------------------------------------------------- restatement
def number(t, v) -> bytes:
    """The bytes of CAST(v AS Utf8): rust_float's digits (Rust 2018 printed -0.0 as "0"; the contract keeps the
    sign, as current Rust does)."""
    if t == BOOL:
        return b"true" if v else b"false"
    if t in (F32, F64):
        x = float(v)
        if x == 0.0 and np.signbit(x):
            return b"-0"
        return rust_float(x, t == F32, False).encode()
    return str(int(v)).encode()


def utf8_field(s: bytes) -> bytes:
    if any(b in SPECIAL for b in s):
        return b'"' + s.replace(b'"', b'""') + b'"'
    return s


def record(fields) -> bytes:
    if len(fields) == 1 and fields[0] == b"":
        return b'""\n'
    return b",".join(fields) + b"\n"


def header(names) -> bytes:
    return record([utf8_field(n.encode("utf-8") if isinstance(n, str) else n) for n in names])


def column_fields(a: Array):
    """One encoded field per row of a host or device Array (a column without validity has no nulls)."""
    a = a.cpu()
    vals, valid = a.numpy_values(), a.valid_mask()
    t = a.data_type
    if t == UTF8:
        return [utf8_field(s) if ok else b"" for s, ok in zip(vals, valid)]
    return [number(t, v) if ok else b"" for v, ok in zip(vals, valid)]


def encode_batch(b: RecordBatch) -> bytes:
    cols = [column_fields(a) for a in b.columns]
    return b"".join(record([c[i] for c in cols]) for i in range(b.num_rows()))


def encode_batches(batches):
    """(the stream, batch_ends) of dfmi_csv_encode_batches over `batches`."""
    parts = [encode_batch(b) for b in batches]
    return b"".join(parts), np.cumsum([len(p) for p in parts], dtype=np.int64).tolist()


# ------------------------------------------------------------- values
def values(t, n, seed):
    """n values of type t: random bit patterns (for floats: NaNs, infinities, subnormals among them) with the
    type's extremes and every decimal length on the even rows."""
    r = np.random.default_rng(seed)
    if t == BOOL:
        return r.integers(0, 2, n).astype(bool)
    if t == UTF8:
        return random_strings(n, seed)
    if t in (F32, F64):
        w = 32 if t == F32 else 64
        bits = r.integers(0, 1 << w, n, dtype=np.uint64)
        out = (bits.astype(np.uint32).view(np.float32) if t == F32 else bits.view(np.float64)).copy()
        tiny = np.finfo(out.dtype).smallest_subnormal
        edge = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 0.1, 1.0, -2.5, 1e21, 1e23, 16777216.0,
                         np.finfo(out.dtype).max, np.finfo(out.dtype).tiny], dtype=out.dtype)
        k = min(n, len(edge))
        out[:k] = edge[:k]
        return out
    dt = np_dtype(t)
    info = np.iinfo(dt)
    edge = [info.min, info.max, 0, 1]
    k = 1
    while k <= info.max:
        edge += [k, k - 1]
        if info.min < 0 and -k >= info.min:
            edge += [-k, -(k - 1)]
        k *= 10
    out = r.integers(0, 1 << 64, n, dtype=np.uint64).astype(dt)  # (wraps into the type)
    even = np.arange(0, n, 2)
    if len(even):
        out[even] = np.array([edge[(i // 2) % len(edge)] for i in even], dtype=dt)
    return out


def random_strings(n, seed, any_byte=True):
    """Short strings, about one in four with a special byte; every byte value when any_byte, else ASCII and
    valid multi-byte UTF-8."""
    r = np.random.default_rng(seed)
    plain = [bytes([c]) for c in range(0x20, 0x7f) if bytes([c]) not in (b'"', b",")]
    if any_byte:
        plain += [bytes([c]) for c in (0x00, 0x01, 0x09, 0x7f)] + [bytes([c]) for c in range(0x80, 0x100)]
    else:
        plain += ["é".encode(), "ß".encode(), "日".encode(), "𝄞".encode(), b"\t"]
    special = [b'"', b",", b"\n", b"\r", b"\r\n", b'""']
    out = []
    for _ in range(n):
        k = int(r.integers(0, 12))
        s = b"".join(plain[int(i)] for i in r.integers(0, len(plain), k))
        if r.random() < 0.25:
            for _ in range(int(r.integers(1, 4))):
                p = int(r.integers(0, len(s) + 1))
                s = s[:p] + special[int(r.integers(0, len(special)))] + s[p:]
        out.append(s)
    return out


# the issue's Utf8 quoting corpus (a 5,000-byte string whose only special byte is its last comes last)
QUOTING = ([b"", None, b'"', b'""', b",", b"\n", b"\r", b"\r\n", b" lead", b"trail ", b"  ", b" , ", b"\x00", b"a\x00b",
            bytes(range(0x80, 0x100)), b"\xff", b"caf\xc3\xa9", b'say "hi"', b"a,b", b"line1\nline2", b"x\ry"] +
           [b'"' * k for k in range(1, 71)] + [b"x" * 4999 + b","])


def _is_utf8(s: bytes) -> bool:
    try:
        s.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


# ... of which Python's csv module over a utf-8 text file (CsvDataSource) can read back: no NUL, valid UTF-8
QUOTING_TEXT = [s for s in QUOTING if s is None or (b"\x00" not in s and _is_utf8(s))]


def some_nulls(n, seed, p=0.3):
    return np.random.default_rng(seed).random(n) >= p


def make_array(t, vals, valid=None) -> Array:
    """A host Array (validity only where a slot is null)."""
    if t == UTF8:
        strs = [None if (s is None or (valid is not None and not valid[i])) else s for i, s in enumerate(vals)]
        return Array.from_strings(strs)
    vals = np.asarray(vals, dtype=bool if t == BOOL else np_dtype(t))
    return Array.from_numpy(t, vals, None if valid is None or np.all(valid) else np.asarray(valid, bool))


def one_type_batch(t, n, seed, nulls=True) -> RecordBatch:
    return RecordBatch(Schema([Field("c", t, True)]), [make_array(t, values(t, n, seed), some_nulls(n, seed + 1)
                                                                  if nulls else None)])


def all_types_batch(n, seed, any_byte=True) -> RecordBatch:
    """n rows of thirteen nullable columns: every type, Utf8 twice (random strings, the quoting corpus cycled)."""
    cols, fields = [], []
    for j, t in enumerate(TYPES):
        v = random_strings(n, seed + j, any_byte) if t == UTF8 else values(t, n, seed + j)
        cols.append(make_array(t, v, some_nulls(n, seed + 50 + j)))
        fields.append(Field("c%d_%s" % (j, t.name.lower()), t, True))
    corpus = QUOTING[:-1] if any_byte else QUOTING_TEXT[:-1]
    cols.append(Array.from_strings([corpus[i % len(corpus)] for i in range(n)]))
    fields.append(Field("quoting", UTF8, True))
    return RecordBatch(Schema(fields), cols)


# ------------------------------------------------------------- the round-trip rule
def assert_reads_back(original, read, what=""):
    """`read` (batches a CSV reader produced from the encoding of `original`) holds the original's rows: valid
    slots bit for bit (NaN: the canonical quiet NaN), equal null counts, a Utf8 null as ""."""
    ncols = original[0].num_columns()
    assert sum(b.num_rows() for b in read) == sum(b.num_rows() for b in original), what
    for c in range(ncols):
        t = original[0].columns[c].data_type
        ov = [a for b in original for a in _rows(b.columns[c])]
        rv = [a for b in read for a in _rows(b.columns[c])]
        if t == UTF8:
            assert [b"" if x is None else x for x in ov] == rv, (what, c)
            continue
        assert [x is None for x in ov] == [x is None for x in rv], (what, c, "nulls")
        for i, (x, y) in enumerate(zip(ov, rv)):
            if x is None:
                continue
            if t in (F32, F64) and x != x:
                x = np.array([np.nan], dtype=np_dtype(t))[0]  # the canonical quiet NaN
                assert _bits(t, x) in (0x7fc00000, 0x7ff8000000000000)
            assert _bits(t, x) == _bits(t, y), (what, c, i, x, y)


def _rows(a: Array):
    a = a.cpu()
    vals, valid = a.numpy_values(), a.valid_mask()
    return [vals[i] if valid[i] else None for i in range(a.length)]


def _bits(t, x) -> int:
    if t == BOOL:
        return int(bool(x))
    return int(np.array([x], dtype=np_dtype(t)).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[
        np.dtype(np_dtype(t)).itemsize])[0])
