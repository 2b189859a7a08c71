"""Writes timestamp_functions.json: the reference's known answers for date_trunc and date_part over Timestamp columns without a time zone, transcribed BY HAND
(data only):
  timestamps.slt  sqllogictest/test_files/timestamps.slt  the zone-free date_trunc rows :979-1262 (literals, the NULL rows, the four ts_data_* tables of :31-46 at
                  'day' and at the four fine granularities, the arrow_cast rows).  :2029-2048 pin only that the result keeps the argument's unit; tests/test_gpu_timestamp.py
                  checks that on every output
  expr.slt        sqllogictest/test_files/expr.slt         the Timestamp rows of date_part / extract, :789-952
  rs              physical-expr/src/datetime_expressions.rs  the vectors of date_trunc_test, :1183-1267 (date_trunc_coarse over nanoseconds)

A case holds `fn`, `arg` (the granularity or part name as the file spells it), `unit` ("s", "ms", "us", "ns"), `ts` (ISO text, null = SQL NULL), `ref`, and
`expected`: ISO text for date_trunc, a number for date_part, null for NULL.  A `TIMESTAMP '...'` literal, to_timestamp(..) and ::timestamp are nanoseconds.
The sqllogictest runner prints a Float64 with its shortest round-trip text, so the date_part numbers are the doubles themselves.
Run: python transcribe_timestamp_functions.py"""
import json
import os

N = None
cases = []
T = "datafusion/sqllogictest/test_files/timestamps.slt:"
E = "datafusion/sqllogictest/test_files/expr.slt:"
R = "datafusion/physical-expr/src/datetime_expressions.rs:"


def case(fn, ref, line, arg, unit, ts, expected):
    cases.append({"name": f"{fn}_{ref.rsplit('/', 1)[1].split('.')[0]}_{line}_{len(cases)}", "fn": fn, "ref": ref + str(line), "arg": arg, "unit": unit, "ts": ts, "expected": expected})


# ---- timestamps.slt :979-1139: every granularity in lower and upper case over one literal, and over NULL
LIT = "2022-08-03T14:38:50"
line = 982
for g, want in (("year", "2022-01-01T00:00:00"), ("quarter", "2022-07-01T00:00:00"), ("month", "2022-08-01T00:00:00"), ("week", "2022-08-01T00:00:00"),
                ("day", "2022-08-03T00:00:00"), ("hour", "2022-08-03T14:00:00"), ("minute", "2022-08-03T14:38:00"), ("second", "2022-08-03T14:38:50")):
    case("date_trunc", T, line, g, "ns", LIT, want)
    case("date_trunc", T, line + 5, g.upper(), "ns", LIT, want)
    case("date_trunc", T, line + 10, g, "ns", N, N)
    case("date_trunc", T, line + 15, g.upper(), "ns", N, N)
    line += 20

# ---- the ts_data tables (:31-46): 1599572549190855123, 1599568949190855123, 1599565349190855123 ns, divided with `/` for the coarser units
ROWS = ["2020-09-08T13:42:29.190855123", "2020-09-08T12:42:29.190855123", "2020-09-08T11:42:29.190855123"]
for unit in ("us", "ms", "ns", "s"):                      # :1143-1162
    for r in ROWS:
        case("date_trunc", T, 1143, "day", unit, r, "2020-09-08T00:00:00")
FINE = {  # unit -> granularity -> the fraction the printed rows keep (:1166-1250)
    "ns": (1166, {"microsecond": ".190855", "millisecond": ".190", "second": "", "minute": N}),
    "us": (1188, {"microsecond": ".190855", "millisecond": ".190", "second": "", "minute": N}),
    "ms": (1210, {"microsecond": ".190", "millisecond": ".190", "second": "", "minute": N}),
    "s": (1232, {"microsecond": "", "millisecond": "", "second": "", "minute": N}),
}
for unit, (ln, grans) in FINE.items():
    for g, frac in grans.items():
        for r in ROWS:
            hm = r[:16]
            case("date_trunc", T, ln, g, unit, r, hm + ":00" if frac is N else hm + ":29" + frac)
# ---- :1256-1266
case("date_trunc", T, 1256, "second", "s", "2023-08-03T14:38:50", "2023-08-03T14:38:50")
case("date_trunc", T, 1258, "second", "ns", "2023-08-03T14:38:50", "2023-08-03T14:38:50")
case("date_trunc", T, 1260, "day", "us", "2023-08-03T14:38:50", "2023-08-03T00:00:00")
case("date_trunc", T, 1262, "day", "ms", "2023-08-03T14:38:50", "2023-08-03T00:00:00")
# ---- datetime_expressions.rs date_trunc_test
V = "2020-09-08T13:42:29.190855"
for ln, ts, g, want in ((1186, V, "second", "2020-09-08T13:42:29"), (1191, V, "minute", "2020-09-08T13:42:00"), (1196, V, "hour", "2020-09-08T13:00:00"),
                        (1201, V, "day", "2020-09-08T00:00:00"), (1206, V, "week", "2020-09-07T00:00:00"), (1211, V, "month", "2020-09-01T00:00:00"),
                        (1216, V, "year", "2020-01-01T00:00:00"), (1222, "2021-01-01T13:42:29.190855", "week", "2020-12-28T00:00:00"),
                        (1227, "2020-01-01T13:42:29.190855", "week", "2019-12-30T00:00:00"), (1233, "2020-01-01T13:42:29.190855", "quarter", "2020-01-01T00:00:00"),
                        (1238, "2020-02-01T13:42:29.190855", "quarter", "2020-01-01T00:00:00"), (1243, "2020-03-01T13:42:29.190855", "quarter", "2020-01-01T00:00:00"),
                        (1248, "2020-04-01T13:42:29.190855", "quarter", "2020-04-01T00:00:00"), (1253, "2020-08-01T13:42:29.190855", "quarter", "2020-07-01T00:00:00"),
                        (1258, "2020-11-01T13:42:29.190855", "quarter", "2020-10-01T00:00:00"), (1263, "2020-12-01T13:42:29.190855", "quarter", "2020-10-01T00:00:00")):
    case("date_trunc", R, ln, g, "ns", ts, want)

# ---- expr.slt: date_part / extract over timestamps
D = "2020-09-08T12:00:00"
for ln, part, ts, want in ((789, "year", D, 2020.0), (799, "quarter", D, 3.0), (809, "month", D, 9.0), (819, "WEEK", D, 37.0), (829, "day", D, 8.0),
                           (839, "doy", D, 252.0), (849, "dow", D, 2.0), (859, "hour", "2020-09-08T12:03:03", 12.0), (864, "minute", "2020-09-08T12:12:00", 12.0),
                           (869, "minute", "2020-09-08T12:12:00", 12.0)):
    case("date_part", E, ln, part, "ns", ts, want)
F = "2020-09-08T12:00:12.12345678"
for ln, part, want in ((874, "second", 12.12345678), (879, "millisecond", 12123.45678), (884, "microsecond", 12123456.78), (889, "nanosecond", 12123456780.0),
                       (895, "second", 12.12345678), (900, "millisecond", 12123.45678), (905, "microsecond", 12123456.78), (910, "nanosecond", 12123456780.0)):
    case("date_part", E, ln, part, "ns", F, want)
case("date_part", E, 937, "epoch", "ns", "1870-01-01T07:29:10.256", -3155646649.744)
case("date_part", E, 942, "epoch", "ns", "2000-01-01T00:00:00", 946684800.0)
case("date_part", E, 947, "epoch", "ns", "2000-01-01T00:00:00", 946684800.0)
case("date_part", E, 952, "epoch", "ns", N, N)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "timestamp_functions.json"), "w", encoding="utf-8") as f:
    json.dump({"cases": cases}, f, indent=1, ensure_ascii=False)
    f.write("\n")
