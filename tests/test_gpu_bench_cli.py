"""bench.py's command line: a plain run times the headline alone, --steps sets
the timed steps, --dump-outputs writes the last step's output columns (whole,
or a fixed seeded sample of a larger output), identical from run to run, and
--full brings back the lines that take runs of their own. The dumped columns
are checked bit for bit against numpy over the oracle's seed-42 table (the
table bench.py generates in HBM): separate multiply and add, one IEEE rounding
per operator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_ffi import gen_unit_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("a", "b", "a_mul_b_plus_c", "sample_rows", "counts")
DUMP_ROWS = 1 << 20  # bench.DUMP_ROWS

pytestmark = pytest.mark.gpu


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


# below DUMP_ROWS selected rows (every row dumped), and above (the sample)
@pytest.mark.parametrize("n", [1_000_003, 4_000_003])
def test_plain_run_and_dump(tmp_path, n):
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    out = _bench("--steps", "3", "--warmup", "1", "--rows", str(n), "--dump-outputs", d1)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "rows/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - n / (out["ms_per_step"] * 1e-3)) <= 1e-9 * out["value"]
    for moved in ("sweep", "parity_gate", "gather", "extra", "cpu_baseline"):
        assert moved not in out
    got = _load(d1)
    a, b, c = (gen_unit_f64(42, j, 0, n) for j in range(3))
    mask = (a > 1.0 - 0.5 ** 0.5) & (b < 0.5 ** 0.5)
    sel = int(mask.sum())
    assert got["counts"].tolist() == [float(n), float(sel)]
    assert (sel > DUMP_ROWS) == (n > 4_000_000)
    rows = got["sample_rows"].astype(np.int64)
    assert rows.size == min(sel, DUMP_ROWS) and rows.min() >= 0 and rows.max() < sel and (np.diff(rows) >= 0).all()
    if sel <= DUMP_ROWS:
        assert np.array_equal(rows, np.arange(sel))
    sa, sb = a[mask][rows], b[mask][rows]
    want = {"a": sa, "b": sb, "a_mul_b_plus_c": (sa * sb) + c[mask][rows]}
    for name, w in want.items():
        assert got[name].dtype == np.float64
        assert np.array_equal(got[name].view(np.uint64), w.view(np.uint64)), name
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= 64 * 1000 * 1000
    if sel > DUMP_ROWS:  # a second run: the same inputs, the same sample, the same bytes
        _bench("--steps", "2", "--warmup", "0", "--rows", str(n), "--dump-outputs", d2)
        again = _load(d2)
        for name in NAMES:
            assert got[name].tobytes() == again[name].tobytes(), name


def test_full_run_has_the_other_lines():
    out = _bench("--steps", "2", "--warmup", "1", "--rows", "1000003", "--full", "--no-cpu", "--sweep", "0.5,0.01",
                 "--extra", "c2i64")
    assert out["full"] is True and out["steps"] == 2
    assert sorted(out["sweep"]) == ["0.01", "0.50"]
    assert out["parity_gate"]["bit_identical_to_oracle"] is True
    assert out["gather"]["checksums_match"] is True
    assert out["extra"]["c2i64"]["parity_gate"]["bit_identical_to_oracle"] is True
    assert "cpu_baseline" not in out
