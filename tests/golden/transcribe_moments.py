"""Writes moments.json: the reference's known answers for VAR_SAMP / VAR_POP / STDDEV_SAMP / STDDEV_POP, transcribed BY HAND (data only):
  variance.rs    physical-expr/src/aggregate/variance.rs:346-506      f64 / i32 / u32 / f32 inputs, one input, NULLs, all NULLs, the two merge tests
  stddev.rs      physical-expr/src/aggregate/stddev.rs:254-432        the same for the standard deviation
  aggregate.slt  sqllogictest/test_files/aggregate.slt:412-416, :1660-1670    stddev over inline values; var / var_pop / stddev / stddev_pop of one and of two values
The queries over aggregate_test_100 (aggregate.slt:370-410) are left out: that CSV file is not part of the reference tree.

A unit-test case holds `kind`, `dtype`, `batches` (lists of values, null = NULL) and `expected` (a Float64 or null).  `merge`: the reference's merge() helper --
batch 0 updates one accumulator, batch 1 another, the second one's state is merged into the first (variance.rs:509-539).  An .slt case holds `values`, the `kinds`
of its output columns and `expected_text`, the cells as the .slt file prints them (floats rounded to 12 decimals, "NULL").       Run: python transcribe_moments.py"""
import json
import os

N = None
SQRT_2 = 1.4142135623730951            # std::f64::consts::SQRT_2
cases = []


def unit(name, ref, kind, dtype, batches, expected, merge=False):
    cases.append({"name": name, "ref": ref, "kind": kind, "dtype": dtype, "batches": batches, "merge": merge, "expected": expected})


def slt(name, ref, values, kinds, expected_text):
    cases.append({"name": name, "ref": ref, "dtype": "float64", "values": values, "kinds": kinds, "expected_text": expected_text})


V = "datafusion/physical-expr/src/aggregate/variance.rs:"
unit("variance_f64_1", V + "346-355", "VAR_POP", "float64", [[1.0, 2.0]], 0.25)
unit("variance_f64_2", V + "357-362", "VAR_POP", "float64", [[1.0, 2.0, 3.0, 4.0, 5.0]], 2.0)
unit("variance_f64_3", V + "364-369", "VAR_SAMP", "float64", [[1.0, 2.0, 3.0, 4.0, 5.0]], 2.5)
unit("variance_f64_4", V + "371-380", "VAR_SAMP", "float64", [[1.1, 2.0, 3.0]], 0.9033333333333333)
unit("variance_i32", V + "382-386", "VAR_POP", "int32", [[1, 2, 3, 4, 5]], 2.0)
unit("variance_u32", V + "388-393", "VAR_POP", "uint32", [[1, 2, 3, 4, 5]], 2.0)
unit("variance_f32", V + "395-400", "VAR_POP", "float32", [[1.0, 2.0, 3.0, 4.0, 5.0]], 2.0)
unit("test_variance_1_input", V + "402-417", "VAR_SAMP", "float64", [[1.0]], N)
unit("variance_i32_with_nulls", V + "419-434", "VAR_POP", "int32", [[1, N, 3, 4, 5]], 2.1875)
unit("variance_i32_all_nulls", V + "436-451", "VAR_SAMP", "int32", [[N, N]], N)
unit("variance_f64_merge_1", V + "453-479", "VAR_POP", "float64", [[1.0, 2.0, 3.0], [4.0, 5.0]], 2.0, merge=True)
unit("variance_f64_merge_2", V + "481-507", "VAR_POP", "float64", [[1.0, 2.0, 3.0, 4.0, 5.0], [N]], 2.0, merge=True)

S = "datafusion/physical-expr/src/aggregate/stddev.rs:"
unit("stddev_f64_1", S + "254-258", "STDDEV_POP", "float64", [[1.0, 2.0]], 0.5)
unit("stddev_f64_2", S + "260-269", "STDDEV_POP", "float64", [[1.1, 2.0, 3.0]], 0.7760297817881877)
unit("stddev_f64_3", S + "271-281", "STDDEV_POP", "float64", [[1.0, 2.0, 3.0, 4.0, 5.0]], SQRT_2)
unit("stddev_f64_4", S + "283-292", "STDDEV_SAMP", "float64", [[1.1, 2.0, 3.0]], 0.9504384952922168)
unit("stddev_i32", S + "294-303", "STDDEV_POP", "int32", [[1, 2, 3, 4, 5]], SQRT_2)
unit("stddev_u32", S + "305-315", "STDDEV_POP", "uint32", [[1, 2, 3, 4, 5]], SQRT_2)
unit("stddev_f32", S + "317-327", "STDDEV_POP", "float32", [[1.0, 2.0, 3.0, 4.0, 5.0]], SQRT_2)
unit("test_stddev_1_input", S + "329-344", "STDDEV_SAMP", "float64", [[1.0]], N)
unit("stddev_i32_with_nulls", S + "346-361", "STDDEV_POP", "int32", [[1, N, 3, 4, 5]], 1.479019945774904)
unit("stddev_i32_all_nulls", S + "363-377", "STDDEV_SAMP", "int32", [[N, N]], N)
unit("stddev_f64_merge_1", S + "379-405", "STDDEV_POP", "float64", [[1.0, 2.0, 3.0], [4.0, 5.0]], SQRT_2, merge=True)
unit("stddev_f64_merge_2", S + "407-433", "STDDEV_POP", "float64", [[1.0, 2.0, 3.0, 4.0, 5.0], [N]], SQRT_2, merge=True)

A = "datafusion/sqllogictest/test_files/aggregate.slt:"
ALL4 = ["VAR_SAMP", "VAR_POP", "STDDEV_SAMP", "STDDEV_POP"]
slt("csv_query_stddev_6", A + "412-416", [1.1, 2.0, 3.0], ["STDDEV_SAMP"], ["0.950438495292"])
slt("variance_single_value", A + "1660-1664", [1.0], ALL4, ["NULL", "0", "NULL", "0"])
slt("variance_two_values", A + "1666-1670", [1.0, 3.0], ALL4, ["2", "1", "1.414213562373", "1"])

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "moments.json"), "w", encoding="utf-8") as f:
    json.dump({"cases": cases}, f, indent=1)
    f.write("\n")
