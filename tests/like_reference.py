"""The checker for LIKE / NOT LIKE / ILIKE / NOT ILIKE: the rules of arrow-string 50.0.0 (what the reference's LikeExpr delegates to) in plain Python.

A pattern is read left to right, one Unicode scalar at a time, and translated into a Python `re`:
  %            any run of characters, the empty run included          -> .*
  _            exactly one Unicode scalar (a line feed too: re.DOTALL)  -> .
  \\% and \\_    that literal character
  \\ + other     a literal backslash; the next character is then read normally (also a backslash ending the pattern)
  other        itself
anchored at both ends (`\\Z`, not `$`, which would let a trailing line feed through).  ILIKE adds re.IGNORECASE, which gives the two non-ASCII scalars whose simple
case folding is ASCII: U+212A (Kelvin sign) matches k, U+017F (long s) matches s.  Python's re.IGNORECASE also lets i match U+0130 / U+0131, which the
reference's simple case folding does not; no test here puts those two scalars into a value.

pyarrow's match_like is NOT the oracle: Arrow C++ lets a backslash escape any character, arrow-rs only `%` and `_`."""
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "like_expr.json")


def like_regex(pattern, case_insensitive=False):
    out, i, n = [], 0, len(pattern)
    while i < n:
        c = pattern[i]
        if c == "%":
            out.append(".*")
        elif c == "_":
            out.append(".")
        elif c == "\\" and i + 1 < n and pattern[i + 1] in "%_":
            out.append(re.escape(pattern[i + 1]))
            i += 1
        else:
            out.append(re.escape(c))
        i += 1
    return re.compile("".join(out) + r"\Z", re.DOTALL | (re.IGNORECASE if case_insensitive else 0))


def like_rows(values, patterns, negated=False, case_insensitive=False):
    """values: list of str / None.  patterns: one str / None for every row (a scalar pattern), or a list of them, one per row.
    -> list of True / False / None: None exactly where the value or the pattern is None."""
    if patterns is None or isinstance(patterns, str):
        patterns = [patterns] * len(values)
    assert len(patterns) == len(values)
    cache, out = {}, []
    for v, p in zip(values, patterns):
        if v is None or p is None:
            out.append(None)
            continue
        rx = cache.get(p)
        if rx is None:
            rx = cache[p] = like_regex(p, case_insensitive)
        out.append((rx.match(v) is not None) != bool(negated))
    return out


def load_goldens():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)["cases"]


def golden_patterns(case):
    """-> (patterns as like_rows takes them, is_scalar)"""
    if "patterns" in case:
        return case["patterns"], False
    return case["pattern"], True


def check_golden(case, rows):
    """rows: one True / False / None per row of case["values"], as computed by whatever is under test"""
    if "expected" in case:
        assert rows == case["expected"], case["name"]
        return
    kept = [v for v, r in zip(case["values"], rows) if r is True]
    if case["rowsort"]:
        kept = sorted(kept)
    assert kept == case["selected"], case["name"]
