"""Writes like_expr.json: the reference's known answers for LIKE / NOT LIKE / ILIKE / NOT ILIKE, transcribed BY HAND (data only):
  like_op        physical-expr/src/expressions/like.rs:216-250             the four vectors of the unit test, one pattern per row (a pattern COLUMN)
  strings.slt    sqllogictest/test_files/strings.slt:18-80                 the five filter queries over the ten-row table
  predicates.slt sqllogictest/test_files/predicates.slt:136-151, :474-492  LIKE '%a%' over strings and over string dictionaries, (s LIKE 'T%') = true
  select.slt     sqllogictest/test_files/select.slt:586-607                column LIKE column, all four forms (the value is LargeUtf8 there; the planner coerces)
  scalar.slt     sqllogictest/test_files/scalar.slt:1718-1731              a NULL pattern and a NULL value, LIKE and NOT LIKE
  binary.slt     sqllogictest/test_files/binary.slt:164-239                LIKE '%F%' over Binary / LargeBinary columns that hold strings (coerced to Utf8)
functions.slt has no LIKE query; predicates.slt:99 and :530 run over files (aggregate_test_100.csv, a Parquet file), not over inline data, and are left out.

A case holds `values`, then either `pattern` (a literal: the scalar form) or `patterns` (one per row), `negated`, `case_insensitive`, and either `expected` (one
Boolean or null per row: a projection) or `selected` (the values of the rows a WHERE keeps; `rowsort`: compared sorted, as the .slt file asks).  `dictionary`: the
reference ran the query over a dictionary-encoded column.       Run: python transcribe_like.py"""
import json
import os

N = None
cases = []


def case(name, ref, values, negated, ci, pattern=None, patterns=None, expected=None, selected=None, rowsort=False, dictionary=False):
    c = {"name": name, "ref": ref, "values": values, "negated": negated, "case_insensitive": ci}
    if patterns is not None:
        c["patterns"] = patterns
    else:
        c["pattern"] = pattern
    if expected is not None:
        c["expected"] = expected
    else:
        c["selected"], c["rowsort"] = selected, rowsort
    if dictionary:
        c["dictionary"] = True
    cases.append(c)


# ---- like.rs:216-250
L = "datafusion/physical-expr/src/expressions/like.rs:"
case("like_op_like", L + "217-224", ["hello world", "world"], False, False, patterns=["%hello%", "%hello%"], expected=[True, False])
case("like_op_not_like", L + "225-232", ["hello world", N, "world"], True, False, patterns=["%hello%", N, "%hello%"], expected=[False, N, True])
case("like_op_ilike", L + "233-240", ["hello world", "world"], False, True, patterns=["%helLo%", "%helLo%"], expected=[True, False])
case("like_op_not_ilike", L + "241-248", ["hello world", N, "world"], True, True, patterns=["%helLo%", N, "%helLo%"], expected=[False, N, True])

# ---- strings.slt
S = "datafusion/sqllogictest/test_files/strings.slt:"
T = ["p1", "p1e1", "p1m1e1", "P1", "P1e1", "P1m1e1", "e1", "p2", "p2e1", "p2m1e1"]
case("strings_like_prefix", S + "35-40", T, False, False, pattern="p1%", selected=["p1", "p1e1", "p1m1e1"], rowsort=True)
case("strings_like_infix", S + "42-47", T, False, False, pattern="%m1%", selected=["P1m1e1", "p1m1e1", "p2m1e1"], rowsort=True)
case("strings_not_like", S + "50-59", T, True, False, pattern="p1%", selected=["P1", "P1e1", "P1m1e1", "e1", "p2", "p2e1", "p2m1e1"], rowsort=True)
case("strings_ilike", S + "63-71", T, False, True, pattern="p1%", selected=["P1", "P1e1", "P1m1e1", "p1", "p1e1", "p1m1e1"], rowsort=True)
case("strings_not_ilike", S + "74-80", T, True, True, pattern="p1%", selected=["e1", "p2", "p2e1", "p2m1e1"], rowsort=True)

# ---- predicates.slt
P = "datafusion/sqllogictest/test_files/predicates.slt:"
case("predicates_like_on_strings", P + "136-144", ["foo", "bar", N, "fazzz"], False, False, pattern="%a%", selected=["bar", "fazzz"])
case("predicates_like_on_string_dictionaries", P + "146-151", ["foo", "bar", N, "fazzz"], False, False, pattern="%a%", selected=["bar", "fazzz"], dictionary=True)
case("predicates_like_equals_true", P + "474-492", ["One", "Two", N, "Four"], False, False, pattern="T%", selected=["Two"])

# ---- select.slt: one row, column1 = 'Bar', column2 = 'B%'
E = "datafusion/sqllogictest/test_files/select.slt:"
case("select_column_like_column", E + "589-592", ["Bar"], False, False, patterns=["B%"], expected=[True])
case("select_column_ilike_column", E + "594-597", ["Bar"], False, True, patterns=["B%"], expected=[True])
case("select_column_not_like_column", E + "599-602", ["Bar"], True, False, patterns=["B%"], expected=[False])
case("select_column_not_ilike_column", E + "604-607", ["Bar"], True, True, patterns=["B%"], expected=[False])

# ---- scalar.slt: values('a'), ('b'), (NULL); `column1 like NULL` and `NULL like column1`
C = "datafusion/sqllogictest/test_files/scalar.slt:"
case("scalar_like_null_pattern", C + "1719-1724", ["a", "b", N], False, False, pattern=N, expected=[N, N, N])
case("scalar_null_like_column", C + "1719-1724", [N, N, N], False, False, patterns=["a", "b", N], expected=[N, N, N])
case("scalar_not_like_null_pattern", C + "1726-1731", ["a", "b", N], True, False, pattern=N, expected=[N, N, N])
case("scalar_null_not_like_column", C + "1726-1731", [N, N, N], True, False, patterns=["a", "b", N], expected=[N, N, N])

# ---- binary.slt: the selected rows print as hex there (466f6f = Foo, 466f6f426172 = FooBar)
Y = "datafusion/sqllogictest/test_files/binary.slt:"
case("binary_like", Y + "228-233", ["Foo", N, "Bar", "FooBar"], False, False, pattern="%F%", selected=["Foo", "FooBar"])
case("largebinary_like", Y + "235-239", ["Foo", N, "Bar", "FooBar"], False, False, pattern="%F%", selected=["Foo", "FooBar"])

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "like_expr.json"), "w", encoding="utf-8") as f:
    json.dump({"cases": cases}, f, indent=1)
    f.write("\n")
