"""A pure-Python restatement, in integer arithmetic, of what the device computes over Timestamp columns: date_part, date_trunc and the casts of dfgpu_cast.
It is the oracle of tests/test_gpu_timestamp.py and is itself pinned to the reference's own answers (tests/golden/timestamp_functions.json) and to
pyarrow.compute by tests/test_timestamp_reference.py.

A timestamp is a Python int counting `unit`s ("s", "ms", "us", "ns") since 1970-01-01T00:00:00, no time zone; None is SQL NULL.  The calendar comes from
datetime.date (proleptic Gregorian, years 1..9999), so nothing here shares code with the kernels' civil-from-days arithmetic.

date_part (datetime_expressions.rs:1019-1142): the instant is split with floor semantics into day number, second of the day and nanosecond of the second;
second .. nanosecond follow to_ticks' operation order in IEEE doubles, epoch is float(value) / float(units per second).
date_trunc (datetime_expressions.rs:429-692): year .. second floor to the period (week: back to Monday); millisecond and microsecond are general_date_trunc's
integer divisions, which truncate toward zero; a granularity as fine as the unit or finer is the identity.  The reference goes through nanoseconds, so an
instant whose value, or whose truncation, does not fit an Int64 of nanoseconds raises OutOfRange.
Casts (arrow-cast 50, safe = false): finer = checked multiply (Overflow), coarser = division toward zero, Date32 <-> Timestamp through units per day."""
import datetime
import json
import os

import scalar_fn_reference as sref

UNITS = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}          # units per second
TYPE_CODE = {"s": 16, "ms": 17, "us": 18, "ns": 19}            # DFGPU_TIMESTAMP_* (include/dfgpu.h)
FN_DATE_PART, FN_DATE_TRUNC = 1, 7                              # DFGPU_FN_*
PARTS = ["year", "quarter", "month", "week", "day", "doy", "dow", "hour", "minute", "second", "millisecond", "microsecond", "nanosecond", "epoch"]
GRANULARITIES = ["year", "quarter", "month", "week", "day", "hour", "minute", "second", "millisecond", "microsecond"]
I64_MIN, I64_MAX = -2**63, 2**63 - 1
EPOCH_ORDINAL = sref.EPOCH_ORDINAL


class OutOfRange(Exception):
    """date_trunc of an instant that, or whose truncation, lies outside 1677-09-21T00:12:43.145224192 .. 2262-04-11T23:47:16.854775807"""


class UnsupportedGranularity(Exception):
    """Unsupported date_trunc granularity: <name>"""


class Overflow(Exception):
    """a cast to a finer unit whose product does not fit an Int64"""


def toward_zero(a, b):
    """Rust's `/` on integers (b > 0)"""
    return a // b if a >= 0 else -((-a) // b)


def window(unit):
    """the values of `unit` whose nanosecond count fits an Int64"""
    ns = 10**9 // UNITS[unit]
    return toward_zero(I64_MIN, ns), toward_zero(I64_MAX, ns)


def split(value, unit):
    """(days, second of the day, nanosecond of the second), all by floor division"""
    sec, sub = divmod(value, UNITS[unit])
    days, sod = divmod(sec, 86400)
    return days, sod, sub * (10**9 // UNITS[unit])


def date_part_ts(part, value, unit):
    if part is None or value is None:
        return None
    p = part.lower()
    if p not in PARTS:
        raise ValueError(f"Date part '{part}' not supported")
    if p == "epoch":
        return float(value) / float(UNITS[unit])
    days, sod, nanos = split(value, unit)
    if p == "hour":
        return float(sod // 3600)
    if p == "minute":
        return float(sod % 3600 // 60)
    if p in ("second", "millisecond", "microsecond", "nanosecond"):
        s = float(sod % 60) + float(nanos) / 1_000_000_000.0
        return s * {"second": 1.0, "millisecond": 1e3, "microsecond": 1e6, "nanosecond": 1e9}[p]
    return sref.date_part(p, days)


def date_trunc(granularity, value, unit):
    if value is None:
        return None
    g = granularity.lower()
    if g not in GRANULARITIES:
        raise UnsupportedGranularity(granularity)
    lo, hi = window(unit)
    if value < lo or value > hi:
        raise OutOfRange(value)
    u = UNITS[unit]
    if g in ("millisecond", "microsecond"):
        per_sec = 10**3 if g == "millisecond" else 10**6
        if u <= per_sec:
            return value
        return toward_zero(value, u // per_sec) * (u // per_sec)
    day = 86400 * u
    fixed = {"day": day, "hour": 3600 * u, "minute": 60 * u, "second": u}
    if g in fixed:
        out = value // fixed[g] * fixed[g]
    else:
        days = value // day
        d = datetime.date.fromordinal(days + EPOCH_ORDINAL)
        if g == "week":
            first = d - datetime.timedelta(days=d.weekday())
        elif g == "month":
            first = d.replace(day=1)
        elif g == "quarter":
            first = d.replace(month=(d.month - 1) // 3 * 3 + 1, day=1)
        else:
            first = d.replace(month=1, day=1)
        out = (first.toordinal() - EPOCH_ORDINAL) * day
    if out < lo:
        raise OutOfRange(value)
    return out


def cast_timestamp(value, from_unit, to_unit):
    if value is None:
        return None
    f, t = UNITS[from_unit], UNITS[to_unit]
    if t >= f:
        out = value * (t // f)
        if not I64_MIN <= out <= I64_MAX:
            raise Overflow(value)
        return out
    return toward_zero(value, f // t)


def date32_to_timestamp(days, unit):
    if days is None:
        return None
    out = days * 86400 * UNITS[unit]
    if not I64_MIN <= out <= I64_MAX:
        raise Overflow(days)
    return out


def timestamp_to_date32(value, unit):
    """value / units per day with Rust's `/`, then `as i32`"""
    if value is None:
        return None
    q = toward_zero(value, 86400 * UNITS[unit]) & 0xFFFFFFFF
    return q - 2**32 if q >= 2**31 else q


def from_iso(text, unit):
    """'2020-09-08T13:42:29.190855123' -> the count in `unit` (digits below the unit are dropped; every text the goldens hold is exact in its unit)"""
    date, _, time = text.partition("T")
    y, m, d = (int(x) for x in date.split("-"))
    hms, _, frac = (time or "00:00:00").partition(".")
    hh, mm, ss = (int(x) for x in hms.split(":"))
    nanos = int((frac + "000000000")[:9]) if frac else 0
    days = datetime.date(y, m, d).toordinal() - EPOCH_ORDINAL
    total_ns = ((days * 86400 + hh * 3600 + mm * 60 + ss) * 10**9) + nanos
    return total_ns // (10**9 // UNITS[unit])


def load_goldens():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timestamp_functions.json")) as f:
        return json.load(f)["cases"]
