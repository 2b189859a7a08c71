"""Writes scalar_functions.json: the reference's known answers for character_length, left, right, starts_with, substr and date_part over Date32,
transcribed BY HAND (data only):
  functions.rs  physical-expr/src/functions.rs   the `test_function!` vectors (only the variants built with the `unicode_expressions` feature): CharacterLength
                :1099-1135, Left :1321-1405, Right :1880-1964, StartsWith :2406-2437, Substr :2620-2845, the negative-length error among them
  expr.slt      sqllogictest/test_files/expr.slt  the Date32 rows of date_part / extract: :783-856 and :956-974 (the rows over timestamps need a Timestamp type and
                are left out)

A case holds `fn` (the function's name), `args` (one entry per argument, null = SQL NULL), `ref`, and either `expected` or `error` (the message's prefix).  Integer
arguments are Int64 (the Int8 literals of two vectors are coerced by the planner); a date is given as ISO text and as days since 1970-01-01 (`days`).
Run: python transcribe_scalar_functions.py"""
import datetime
import json
import os

N = None
cases = []
F = "datafusion/physical-expr/src/functions.rs:"
E = "datafusion/sqllogictest/test_files/expr.slt:"


def case(fn, line, args, expected=None, error=None, ref=F):
    c = {"name": f"{fn}_{line}", "fn": fn, "ref": ref + str(line), "args": args}
    if error is not None:
        c["error"] = error
    else:
        c["expected"] = expected
    cases.append(c)


# ---- CharacterLength
case("character_length", 1100, ["chars"], 5)
case("character_length", 1109, ["josé"], 4)
case("character_length", 1118, [""], 0)
case("character_length", 1127, [N], N)

# ---- Left
case("left", 1322, ["abcde", 2], "ab")
case("left", 1331, ["abcde", 200], "abcde")
case("left", 1340, ["abcde", -2], "abc")
case("left", 1349, ["abcde", -200], "")
case("left", 1358, ["abcde", 0], "")
case("left", 1367, [N, 2], N)
case("left", 1379, ["abcde", N], N)
case("left", 1388, ["joséésoj", 5], "joséé")
case("left", 1397, ["joséésoj", -3], "joséé")

# ---- Right
case("right", 1881, ["abcde", 2], "de")
case("right", 1890, ["abcde", 200], "abcde")
case("right", 1899, ["abcde", -2], "cde")
case("right", 1908, ["abcde", -200], "")
case("right", 1917, ["abcde", 0], "")
case("right", 1926, [N, 2], N)
case("right", 1938, ["abcde", N], N)
case("right", 1947, ["joséésoj", 5], "éésoj")
case("right", 1956, ["joséésoj", -3], "éésoj")

# ---- StartsWith
case("starts_with", 2407, ["alphabet", "alph"], True)
case("starts_with", 2415, ["alphabet", "blph"], False)
case("starts_with", 2423, [N, "alph"], N)
case("starts_with", 2431, ["alphabet", N], N)

# ---- Substr
case("substr", 2621, ["alphabet", 0], "alphabet")
case("substr", 2630, ["joséésoj", 5], "ésoj")
case("substr", 2639, ["joséésoj", -5], "joséésoj")
case("substr", 2648, ["alphabet", 1], "alphabet")
case("substr", 2657, ["alphabet", 2], "lphabet")
case("substr", 2666, ["alphabet", 3], "phabet")
case("substr", 2675, ["alphabet", -3], "alphabet")
case("substr", 2684, ["alphabet", 30], "")
case("substr", 2693, ["alphabet", N], N)
case("substr", 2702, ["alphabet", 3, 2], "ph")
case("substr", 2715, ["alphabet", 3, 20], "phabet")
case("substr", 2728, ["alphabet", 0, 5], "alph")
case("substr", 2742, ["alphabet", -5, 10], "alph")
case("substr", 2756, ["alphabet", -5, 4], "")
case("substr", 2770, ["alphabet", -5, 5], "")
case("substr", 2783, ["alphabet", N, 20], N)
case("substr", 2796, ["alphabet", 3, N], N)
case("substr", 2809, ["alphabet", 1, -1], error="negative substring length not allowed")
case("substr", 2822, ["joséésoj", 5, 2], "és")


# ---- expr.slt: date_part(part, CAST(... AS DATE)) and extract(epoch from arrow_cast(.., 'Date32'))
def date_case(line, part, iso, expected):
    days = (datetime.date.fromisoformat(iso) - datetime.date(1970, 1, 1)).days
    c = {"name": f"date_part_{line}", "fn": "date_part", "ref": E + str(line), "args": [part, iso], "days": days, "expected": float(expected)}
    cases.append(c)


date_case(784, "YEAR", "2000-01-01", 2000)
date_case(794, "QUARTER", "2000-01-01", 1)
date_case(804, "MONTH", "2000-01-01", 1)
date_case(814, "WEEK", "2003-01-01", 1)
date_case(824, "DAY", "2000-01-01", 1)
date_case(834, "DOY", "2000-01-01", 1)
date_case(844, "DOW", "2000-01-01", 6)
date_case(854, "HOUR", "2000-01-01", 0)
date_case(957, "epoch", "1970-01-01", 0)
date_case(962, "epoch", "1970-01-02", 86400)
date_case(967, "epoch", "1970-01-11", 864000)
date_case(972, "epoch", "1969-12-31", -86400)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "scalar_functions.json"), "w", encoding="utf-8") as f:
    json.dump({"cases": cases}, f, indent=1, ensure_ascii=False)
    f.write("\n")
