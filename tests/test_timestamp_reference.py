"""tests/timestamp_reference.py -- the oracle of the device's Timestamp tests -- against the reference's own answers (tests/golden/timestamp_functions.json),
against pyarrow.compute wherever pyarrow defines the same thing, and against hand-written cases of general_date_trunc's formulas; and the type codes of
include/dfgpu.h against their mirrors in capi.py and shim/src/ffi.rs.  No device."""
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import timestamp_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ref.load_goldens()
CODES = {"DFGPU_TIMESTAMP_SECOND": 16, "DFGPU_TIMESTAMP_MILLISECOND": 17, "DFGPU_TIMESTAMP_MICROSECOND": 18, "DFGPU_TIMESTAMP_NANOSECOND": 19, "DFGPU_FN_DATE_TRUNC": 7}


def test_type_codes_agree_in_header_python_and_rust():
    header = open(os.path.join(ROOT, "include", "dfgpu.h")).read()
    rust = open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read()
    from dfgpu import capi
    for name, value in CODES.items():
        assert re.search(rf"\b{name} = {value}\b", header), f"include/dfgpu.h does not declare {name} = {value}"
        assert re.search(rf"\bpub const {name}: i32 = {value};", rust), f"shim/src/ffi.rs does not declare {name} = {value}"
        assert getattr(capi, name[len("DFGPU_"):]) == value
    assert ref.TYPE_CODE == {"s": 16, "ms": 17, "us": 18, "ns": 19} and ref.FN_DATE_TRUNC == 7


def test_goldens_are_all_here():
    assert len(GOLDENS) == 134 and {c["fn"] for c in GOLDENS} == {"date_trunc", "date_part"}


@pytest.mark.parametrize("case", GOLDENS, ids=[c["name"] for c in GOLDENS])
def test_restatement_reproduces_the_reference(case):
    value = None if case["ts"] is None else ref.from_iso(case["ts"], case["unit"])
    if case["fn"] == "date_trunc":
        want = None if case["expected"] is None else ref.from_iso(case["expected"], case["unit"])
        assert ref.date_trunc(case["arg"], value, case["unit"]) == want
    else:
        got = ref.date_part_ts(case["arg"], value, case["unit"])
        assert got == case["expected"] and (got is None or isinstance(got, float))


def instants(unit, n=1500, seed=5):
    """random instants inside the nanosecond window, both sides of 1970, and the window's edges"""
    lo, hi = ref.window(unit)
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(lo, hi, n, dtype=np.int64)] + [lo, hi, -1, 0, 1]


@pytest.mark.parametrize("unit", list(ref.UNITS))
def test_components_agree_with_pyarrow(unit):
    vals = instants(unit)
    a = pa.array(vals, type=pa.int64()).cast(pa.timestamp(unit))
    # second / subsecond fields as integers: what the float parts are assembled from
    got = [ref.split(v, unit) for v in vals]
    assert [g[1] // 3600 for g in got] == pc.hour(a).to_pylist()
    assert [g[1] % 3600 // 60 for g in got] == pc.minute(a).to_pylist()
    assert [g[1] % 60 for g in got] == pc.second(a).to_pylist()
    assert [g[2] for g in got] == [ms * 10**6 + us * 10**3 + ns for ms, us, ns in zip(pc.millisecond(a).to_pylist(), pc.microsecond(a).to_pylist(), pc.nanosecond(a).to_pylist())]
    for part, fn in (("year", pc.year), ("quarter", pc.quarter), ("month", pc.month), ("day", pc.day), ("doy", pc.day_of_year), ("week", pc.iso_week),
                     ("hour", pc.hour), ("minute", pc.minute)):
        assert [ref.date_part_ts(part, v, unit) for v in vals] == [float(x) for x in fn(a).to_pylist()], part
    sunday0 = pc.day_of_week(a, count_from_zero=True, week_start=7).to_pylist()
    assert [ref.date_part_ts("dow", v, unit) for v in vals] == [float(x) for x in sunday0]


@pytest.mark.parametrize("unit", list(ref.UNITS))
@pytest.mark.parametrize("gran", ["year", "quarter", "month", "week", "day", "hour", "minute", "second"])
def test_floor_granularities_agree_with_pyarrow(unit, gran):
    lo, hi = ref.window(unit)
    vals, want = [], []
    week = 7 * 86400 * ref.UNITS[unit]
    for v in instants(unit, seed=11):
        if gran == "week" and v > hi - week:          # pyarrow shifts the instant by the week's start before it floors: within days of the upper edge that sum wraps
            continue
        try:
            want.append(ref.date_trunc(gran, v, unit))
            vals.append(v)
        except ref.OutOfRange:
            assert v // (86400 * ref.UNITS[unit]) <= lo // (86400 * ref.UNITS[unit]) + 366          # only next to the window's lower edge
    a = pa.array(vals, type=pa.int64()).cast(pa.timestamp(unit))
    got = pc.floor_temporal(a, 1, gran, week_starts_monday=True).cast(pa.int64()).to_pylist()
    assert got == want and len(vals) > 1400


def test_sub_second_granularities_truncate_toward_zero():
    """general_date_trunc, datetime_expressions.rs:581-604: `nano / 1_000 / 1_000 * 1_000` and its siblings are Rust integer divisions"""
    assert ref.date_trunc("millisecond", -1500, "us") == -1000 and ref.date_trunc("second", -1500, "ms") == -2000          # toward zero vs floor
    assert ref.date_trunc("millisecond", 1500, "us") == 1000 and ref.date_trunc("second", 1500, "ms") == 1000
    assert ref.date_trunc("millisecond", -1, "ns") == 0 and ref.date_trunc("microsecond", -1, "ns") == 0 and ref.date_trunc("second", -1, "ns") == -10**9
    assert ref.date_trunc("microsecond", -1_999, "ns") == -1_000 and ref.date_trunc("millisecond", -1_999_999, "ns") == -1_000_000
    assert ref.date_trunc("millisecond", -2_000_000, "ns") == -2_000_000
    for unit, gran in (("s", "millisecond"), ("s", "microsecond"), ("ms", "millisecond"), ("ms", "microsecond"), ("us", "microsecond")):          # as fine as the unit: identity
        for v in (-1501, -1, 0, 1, 1501):
            assert ref.date_trunc(gran, v, unit) == v
    assert ref.date_trunc("MilliSecond", -1500, "us") == -1000
    with pytest.raises(ref.UnsupportedGranularity):
        ref.date_trunc("fortnight", 0, "s")
    assert ref.date_trunc("fortnight", None, "s") is None


def test_window_edges():
    for unit in ref.UNITS:
        lo, hi = ref.window(unit)
        ns = 10**9 // ref.UNITS[unit]
        assert ref.I64_MIN <= lo * ns and (lo - 1) * ns < ref.I64_MIN and hi * ns <= ref.I64_MAX < (hi + 1) * ns
        assert ref.date_trunc("microsecond", lo, unit) in (lo, lo // 1000 * 1000 + 1000) and ref.date_trunc("second", hi, unit) == hi // ref.UNITS[unit] * ref.UNITS[unit]
        for v in (lo - 1, hi + 1):
            with pytest.raises(ref.OutOfRange):
                ref.date_trunc("microsecond", v, unit)
        with pytest.raises(ref.OutOfRange):          # 1677-09-21T00:00:00 lies below the window
            ref.date_trunc("day", lo, unit)
    assert ref.from_iso("1677-09-21T00:12:43.145224192", "ns") == ref.I64_MIN and ref.from_iso("2262-04-11T23:47:16.854775807", "ns") == ref.I64_MAX


def test_casts():
    assert ref.cast_timestamp(-1500, "ms", "s") == -1 and ref.cast_timestamp(1500, "ms", "s") == 1 and ref.cast_timestamp(-1, "ns", "s") == 0
    assert ref.cast_timestamp(-7, "s", "ns") == -7 * 10**9 and ref.cast_timestamp(5, "us", "us") == 5
    with pytest.raises(ref.Overflow):
        ref.cast_timestamp(ref.I64_MAX // 10**9 + 1, "s", "ns")
    assert ref.cast_timestamp(ref.I64_MAX // 10**9, "s", "ns") == ref.I64_MAX // 10**9 * 10**9
    assert ref.date32_to_timestamp(-1, "ms") == -86_400_000 and ref.date32_to_timestamp(2**31 - 1, "ms") == (2**31 - 1) * 86400 * 10**3
    with pytest.raises(ref.Overflow):          # beyond day 106751991 the microsecond count leaves an Int64 too
        ref.date32_to_timestamp(106751992, "us")
    with pytest.raises(ref.Overflow):
        ref.date32_to_timestamp(106752, "ns")
    assert ref.date32_to_timestamp(106751, "ns") == 106751 * 86400 * 10**9
    assert ref.timestamp_to_date32(-86400, "s") == -1 and ref.timestamp_to_date32(-86399, "s") == 0 and ref.timestamp_to_date32(86399_999, "ms") == 0
    assert ref.timestamp_to_date32(ref.I64_MAX, "s") == (ref.I64_MAX // 86400) % 2**32 - (2**32 if (ref.I64_MAX // 86400) % 2**32 >= 2**31 else 0)
    # pyarrow agrees on the casts it defines without error: finer units, and coarser units of exact multiples
    vals = [-86400 * 3, -1, 0, 59, 86400 * 365]
    a = pa.array(vals, type=pa.int64()).cast(pa.timestamp("s"))
    assert a.cast(pa.timestamp("us")).cast(pa.int64()).to_pylist() == [ref.cast_timestamp(v, "s", "us") for v in vals]
    exact = pa.array([v * 1000 for v in vals], type=pa.int64()).cast(pa.timestamp("ms"))
    assert exact.cast(pa.timestamp("s")).cast(pa.int64()).to_pylist() == [ref.cast_timestamp(v * 1000, "ms", "s") for v in vals] == vals
    days = pa.array([-3, 0, 365], type=pa.int32()).cast(pa.date32())
    assert days.cast(pa.timestamp("ms")).cast(pa.int64()).to_pylist() == [ref.date32_to_timestamp(d, "ms") for d in (-3, 0, 365)]
