"""What tests/test_gpu_group_normalize.py rests on, checked without a GPU: the
crafted tables cancel the way they are built to, the oracle's sums over them
are the exact rational sums rounded once (so the reference is right
independently of any device), the restatements the device tests assert with
(the trip rule, the normalised digit string, SUM's and AVG's bits) hold on
hand cases, the library exports the trip counter, and DESIGN.md names the
knob. The oracle executes no AVG: an AVG's bits are the contract's
(test_avg_cpu.avg_bits), checked here against the rational quotient."""
import ctypes as C
import math
import subprocess
import sys
from fractions import Fraction

import numpy as np

from datafusion_amd import _abi
from test_aggregate_cpu import bits_f32, bits_f64
from test_avg_cpu import F_NAN, F_NINF, F_PINF, LIMBS, ROOT, UNIT, avg_bits, f32_round
from test_gpu_group_normalize import (CRAFTED_WANT, NORM_ROWS, X, Y, crafted_table, digits_of, high_low_table,
                                      rule_trips, sum_bits, value_of)


def rounded_once(q: Fraction, f32: bool) -> int:
    """The bits of an exact rational rounded half to even to Float32 / Float64 (test_avg_cpu's helper below the
    format's overflow threshold: the largest finite value plus half its last place)."""
    big = Fraction(2 ** 128 - 2 ** 103) if f32 else Fraction(2 ** 1024 - 2 ** 970)
    if abs(q) >= big:
        v = math.inf if q > 0 else -math.inf
        return bits_f32(v) if f32 else bits_f64(v)
    if f32:
        return bits_f32(f32_round(q))
    v = float(q)  # int / int true division: correctly rounded, subnormals included
    return bits_f64(-0.0 if v == 0.0 and q < 0 else v)


def want_bits(w, f32: bool):
    if w is None:
        return None
    if w != w:
        return 0x7FC00000 if f32 else 0x7FF8000000000000
    return bits_f32(w) if f32 else bits_f64(w)


def test_crafted_groups_cancel_as_stated():
    """Every crafted group's exact sums are the stated ones, in both columns; each (but the late arrival and the
    probe rows) has rows in at least two batches with one in A, so a pass falls between them whether it runs
    before every batch or once before C."""
    t = crafted_table()
    ex = t.exact()
    crafted = {nm: g for nm, g in t.names.items() if not nm.startswith(b"f")}
    assert set(crafted) == set(CRAFTED_WANT)
    s = t.starts()
    for nm, g in crafted.items():
        for c in (X, Y):
            n, total, flags = ex[g][c - X]
            assert sum_bits(total, n, c == Y, flags) == want_bits(CRAFTED_WANT[nm][c - X], c == Y), (nm, c)
        rows = np.nonzero(t.gid == g)[0]
        batches = {max(b for b in range(5) if s[b] <= i) for i in rows}
        if nm not in (b"late_arrival", b"probe-a", b"probe-b"):
            # (over_and_back is back after batch B: only a pass before every batch falls inside it; its _late twin
            # stays past the finite range until D)
            assert 0 in batches and len(batches) >= 2 and (max(batches) >= 2 or nm == b"over_and_back"), nm
    assert set(np.nonzero(t.gid == crafted[b"late_arrival"])[0]) <= set(range(s[3], s[4]))
    # the hidden terms and the survivors lie far below what the cancelled high parts would round away
    assert ex[crafted[b"ripple_zero"]][0][1] == 0 and ex[crafted[b"heavy"]][0][1] == 5
    assert digits_of(-1) == (0xffffffff,) * (LIMBS - 1) + (-1,)  # the state of a ripple group after batch A


def test_oracle_sums_are_the_rationals_rounded_once():
    """The oracle over the crafted table (grouped by the Utf8 key, which names the group): SUM(x) and SUM(y) of
    every group, filler included, equal the exact rational sum rounded once, and the restatement the device
    tests use (sum_bits) agrees; the AVG restatement equals the rational quotient rounded once."""
    t = crafted_table()
    rk, rv, rs = t.oracle("utf8")
    ex = t.exact()
    assert len(rk) == len(ex)
    seen = set()
    for g, name in enumerate(rs[0]):
        gid = -1 if name is None else t.names[name]
        seen.add(gid)
        for j, c in ((0, X), (2, Y)):  # AGGS: SUM(x) first, SUM(y) third
            n, total, flags = ex[gid][c - X]
            v = rv[g][j]
            assert int(v.count) == n and bool(v.is_null) == (n == 0), (name, c)
            if n == 0:
                continue
            if flags & F_NAN or (flags & F_PINF and flags & F_NINF):
                want = 0x7FC00000 if c == Y else 0x7FF8000000000000
            elif flags & (F_PINF | F_NINF):
                want = want_bits(math.inf if flags & F_PINF else -math.inf, c == Y)
            elif total == 0:
                want = sum_bits(total, n, c == Y, flags)  # (the zero's sign: the contract's rule)
            else:
                want = rounded_once(Fraction(total, 1 << UNIT), c == Y)
                assert avg_bits(total, n, c == Y, flags) == rounded_once(Fraction(total, n << UNIT), c == Y), (name, c)
            assert int(v.bits) == want == sum_bits(total, n, c == Y, flags), (name, c, hex(int(v.bits)), hex(want))
    assert seen == set(ex)


def test_high_low_tables_hold_a_negative_sum_in_every_group():
    t = high_low_table(600, 900)
    ex = t.exact()
    assert len(ex) == 1502 and t.counts == [1200, 2400, 1500, 2]
    for g, e in ex.items():
        if t.name_of[g].startswith(b"g"):
            assert e[0][1] < 0 and e[1][1] < 0 and e[0][0] == e[1][0] >= 3
        else:
            assert e[0][0] == e[1][0] == 0
    # after batch 0 the low terms are hidden: the first groups' sums round to the high term alone
    first = t.exact(t.counts[0])
    assert all(sum_bits(e[0][1], e[0][0], False, e[0][2]) == bits_f64(2.0 ** 900) for e in first.values())


def test_restatements_on_hand_cases():
    # the trip rule: r + m > T trips before the batch is added, an empty batch is skipped
    assert rule_trips([5, 5, 5], 0) == (3, 5)
    assert rule_trips([5, 5, 5], 10) == (1, 5)
    assert rule_trips([5, 0, 5, 1], 10) == (1, 1)
    assert rule_trips([5, 5, 5], 15) == (0, 15)
    assert rule_trips([5, 5, 5], 0, float_sum=False) == (0, 15)
    assert rule_trips([1 << 29, 1 << 29, 1], NORM_ROWS) == (1, 1)
    # digits: floor carries, the top digit signed
    for total in (0, 1, -1, 2 ** 32, -2 ** 32, -2 ** 32 - 1, 2 ** 2100 - 1, -(2 ** 2100) + 12345, 3 << 2098):
        d = digits_of(total)
        assert len(d) == LIMBS and value_of(d) == total and all(0 <= x < 2 ** 32 for x in d[:-1])
    assert digits_of(-3)[0] == 0xfffffffd and digits_of(-3)[-1] == -1
    # a sum at the overflow threshold is an infinity, one quantum of the 2^-1074 grid below it the largest value
    lim = (2 ** 1024 - 2 ** 970) << UNIT
    assert sum_bits(lim, 3, False, 8) == bits_f64(math.inf) and sum_bits(-lim, 3, False, 8) == bits_f64(-math.inf)
    assert sum_bits(lim - 1, 3, False, 8) == bits_f64(float(np.finfo(np.float64).max))
    lim = (2 ** 128 - 2 ** 103) << UNIT
    assert sum_bits(lim, 3, True, 8) == bits_f32(math.inf)
    assert sum_bits(lim - 1, 3, True, 8) == bits_f32(float(np.finfo(np.float32).max))
    assert sum_bits(0, 0, False, 0) is None


def test_trip_counter_is_exported_and_starts_at_zero():
    """dfmi_internal_group_normalize_trips: exported by the built library, 0 in a fresh process (this test is about
    that process); dfmi_internal_group_records next to it."""
    code = ("import ctypes as C; L = C.CDLL(%r); f = L.dfmi_internal_group_normalize_trips; f.restype = C.c_long; "
            "assert L.dfmi_internal_group_records; print(f())" % _abi.LIB_PATH)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "0"
    f = _abi.lib().dfmi_internal_group_normalize_trips
    f.restype = C.c_long
    assert f() >= 0


def test_design_names_the_knob_and_the_counter():
    import os
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    for word in ("DFMI_GROUP_NORM_ROWS", "dfmi_internal_group_normalize_trips", "dfmi_internal_group_records",
                 "DFMI_GROUP_GRID", "dfmi_internal_group_strided_launches", "test_gpu_groupby_stride.py"):
        assert word in text, word


def test_strided_launch_counter_is_exported_and_starts_at_zero():
    """dfmi_internal_group_strided_launches (groupby.h "Diagnostic grid cap"): exported by the built library and 0
    in a fresh process, with or without the grid knob in its environment -- nothing counts before a launch."""
    import os
    code = ("import ctypes as C; L = C.CDLL(%r); f = L.dfmi_internal_group_strided_launches; f.restype = C.c_long; "
            "print(f())" % _abi.LIB_PATH)
    for knobs in ({}, {"DFMI_DIAG": "1", "DFMI_GROUP_GRID": "3"}):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, **knobs))
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip() == "0"
