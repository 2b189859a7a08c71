"""A pure-Python restatement of the scalar functions the device evaluates (dfgpu_scalar_function), the oracle of tests/test_gpu_scalar_fn.py.  It is pinned to
the reference's own known answers (tests/golden/scalar_functions.json) by tests/test_scalar_fn_reference.py.

Dates are days since 1970-01-01 in the proleptic Gregorian calendar (datetime.date.fromordinal(days + 719163)); strings are Python str, whose indices count code
points as the reference's `chars()` does.  None is SQL NULL: a NULL in any argument gives NULL."""
import datetime
import json
import os

FN = {"date_part": 1, "character_length": 2, "substr": 3, "left": 4, "right": 5, "starts_with": 6}          # DFGPU_FN_* (include/dfgpu.h)
PARTS = ["year", "quarter", "month", "week", "day", "doy", "dow", "hour", "epoch"]
UNSUPPORTED_PARTS = ["minute", "second", "millisecond", "microsecond", "nanosecond"]                    # nothing pins them for Date32
EPOCH_ORDINAL = 719163          # datetime.date(1970, 1, 1).toordinal()
MIN_DAY, MAX_DAY = 1 - EPOCH_ORDINAL, datetime.date.max.toordinal() - EPOCH_ORDINAL                     # 0001-01-01 .. 9999-12-31


class NegativeSubstringLength(Exception):
    """substr(s, start, count < 0) on a row whose three arguments are non-NULL: `negative substring length not allowed`"""


def date_part(part, days):
    if part is None or days is None:
        return None
    p = part.lower()
    if p not in PARTS:
        raise ValueError(f"Date part '{part}' not supported")
    d = datetime.date.fromordinal(days + EPOCH_ORDINAL)
    if p == "year":
        return float(d.year)
    if p == "quarter":
        return float((d.month - 1) // 3 + 1)
    if p == "month":
        return float(d.month)
    if p == "week":
        return float(d.isocalendar()[1])
    if p == "day":
        return float(d.day)
    if p == "doy":
        return float(d.timetuple().tm_yday)
    if p == "dow":
        return float((d.weekday() + 1) % 7)
    if p == "hour":
        return 0.0
    return days * 86400.0


def character_length(s):
    return None if s is None else len(s)


def substr(s, start, count=0, three=False):
    if s is None or start is None or (three and count is None):
        return None
    if not three:
        return s if start <= 0 else s[start - 1:]
    if count < 0:
        raise NegativeSubstringLength(f"negative substring length not allowed: substr(<str>, {start}, {count})")
    skip = max(0, start - 1)
    take = max(0, count + (start - 1 if start < 1 else 0))
    return s[skip:skip + take]


def left(s, n):
    if s is None or n is None:
        return None
    if n > 0:
        return s[:n]
    if n == 0:
        return ""
    return s[:max(0, len(s) + n)]


def right(s, n):
    if s is None or n is None:
        return None
    if n > 0:
        return s[max(0, len(s) - n):]
    if n == 0:
        return ""
    return s[min(len(s), -n):]


def starts_with(s, p):
    if s is None or p is None:
        return None
    return s.encode().startswith(p.encode())


def evaluate(fn, args):
    """one row: fn by name, args as the golden file lists them"""
    if fn == "date_part":
        return date_part(args[0], args[1])
    if fn == "character_length":
        return character_length(args[0])
    if fn == "substr":
        return substr(args[0], args[1], args[2] if len(args) == 3 else 0, len(args) == 3)
    if fn == "left":
        return left(args[0], args[1])
    if fn == "right":
        return right(args[0], args[1])
    if fn == "starts_with":
        return starts_with(args[0], args[1])
    raise ValueError(fn)


def rows(fn, columns):
    """columns: one list per argument, all of one length -> one result per row"""
    return [evaluate(fn, list(r)) for r in zip(*columns)]


def load_goldens():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar_functions.json"), encoding="utf-8") as f:
        return json.load(f)["cases"]


def golden_args(case):
    """the arguments as `evaluate` takes them: a date_part case carries its date as days since the epoch"""
    return [case["args"][0], case["days"]] if case["fn"] == "date_part" else list(case["args"])
