"""Writes comoments.json: the reference's known answers for COVAR_SAMP / COVAR_POP / CORR / REGR_*, transcribed BY HAND (data only):
  covariance.rs   physical-expr/src/aggregate/covariance.rs:419-742     f64 / i32 / u32 / f32 inputs, NULLs in either argument, all NULLs, one input, the two merge tests
  correlation.rs  physical-expr/src/aggregate/correlation.rs:259-494    the same for the correlation
  aggregate.slt   sqllogictest/test_files/aggregate.slt:264-305 (covar), :314-350 (corr), :2805-2910 (regr_*: NULL results, the constant-x case, the basic case, NULLs ignored)
The queries over aggregate_test_100 (aggregate.slt:246-262, :308-312, :2849-2862) are left out: that CSV file is not part of the reference tree.

A unit-test case holds `kind`, the two `dtypes`, `batches` (pairs of value lists [a, b], null = NULL) and `expected` (a Float64 or null).  `merge`: the reference's
merge() helper -- batch 0 updates one accumulator, batch 1 another, the second one's state is merged into the first (covariance.rs:744-765).  An .slt case holds the
value lists `a` and `b` (argument 0 and argument 1 of every aggregate of the query), the `kinds` of its output columns and `expected_text`, the cells as the .slt file
prints them (floats rounded to 12 decimals, "NULL").       Run: python transcribe_comoments.py"""
import json
import os

N = None
cases = []


def unit(name, ref, kind, dtype, batches, expected, merge=False):
    cases.append({"name": name, "ref": ref, "kind": kind, "dtypes": [dtype, dtype], "batches": batches, "merge": merge, "expected": expected})


def slt(name, ref, dtype, a, b, kinds, expected_text):
    cases.append({"name": name, "ref": ref, "dtypes": [dtype, dtype], "a": a, "b": b, "kinds": kinds, "expected_text": expected_text.split()})


V = "datafusion/physical-expr/src/aggregate/covariance.rs:"
unit("covariance_f64_1", V + "419-432", "COVAR_POP", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]], 0.6666666666666666)
unit("covariance_f64_2", V + "434-447", "COVAR_SAMP", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]], 1.0)
unit("covariance_f64_4", V + "449-462", "COVAR_SAMP", "float64", [[[1.1, 2.0, 3.0], [4.1, 5.0, 6.0]]], 0.9033333333333335)
unit("covariance_f64_5", V + "464-477", "COVAR_POP", "float64", [[[1.1, 2.0, 3.0], [4.1, 5.0, 6.0]]], 0.6022222222222223)
unit("covariance_f64_6", V + "479-496", "COVAR_POP", "float64", [[[1.0, 2.0, 3.0, 1.1, 2.2, 3.3], [4.0, 5.0, 6.0, 4.4, 5.5, 6.6]]], 0.7616666666666666)
unit("covariance_i32", V + "498-511", "COVAR_POP", "int32", [[[1, 2, 3], [4, 5, 6]]], 0.6666666666666666)
unit("covariance_u32", V + "513-525", "COVAR_POP", "uint32", [[[1, 2, 3], [4, 5, 6]]], 0.6666666666666666)
unit("covariance_f32", V + "527-539", "COVAR_POP", "float32", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]], 0.6666666666666666)
unit("covariance_i32_with_nulls_1", V + "541-554", "COVAR_POP", "int32", [[[1, N, 3], [4, N, 6]]], 1.0)
unit("covariance_i32_with_nulls_2", V + "556-583", "COVAR_POP", "int32", [[[1, N, 2, N, 3, N], [4, 9, 5, 8, 6, N]]], 0.6666666666666666)
unit("covariance_i32_with_nulls_3", V + "585-612", "COVAR_SAMP", "int32", [[[1, N, 2, N, 3, N], [4, 9, 5, 8, 6, N]]], 1.0)
unit("covariance_i32_all_nulls", V + "614-627", "COVAR_SAMP", "int32", [[[N, N], [N, N]]], N)
unit("covariance_pop_i32_all_nulls", V + "629-642", "COVAR_POP", "int32", [[[N, N], [N, N]]], N)
unit("covariance_1_input", V + "644-657", "COVAR_SAMP", "float64", [[[1.0], [2.0]]], N)
unit("covariance_pop_1_input", V + "659-672", "COVAR_POP", "float64", [[[1.0], [2.0]]], 0.0)
unit("covariance_f64_merge_1", V + "674-707", "COVAR_POP", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [[1.1, 2.2, 3.3], [4.4, 5.5, 6.6]]], 0.7616666666666666, merge=True)
unit("covariance_f64_merge_2", V + "709-742", "COVAR_POP", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [[N], [N]]], 0.6666666666666666, merge=True)

R = "datafusion/physical-expr/src/aggregate/correlation.rs:"
unit("correlation_f64_1", R + "259-272", "CORR", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 7.0]]], 0.9819805060619659)
unit("correlation_f64_2", R + "274-287", "CORR", "float64", [[[1.0, 2.0, 3.0], [4.0, -5.0, 6.0]]], 0.17066403719657236)
unit("correlation_f64_4", R + "289-302", "CORR", "float64", [[[1.1, 2.0, 3.0], [4.1, 5.0, 6.0]]], 1.0)
unit("correlation_f64_6", R + "304-321", "CORR", "float64", [[[1.0, 2.0, 3.0, 1.1, 2.2, 3.3], [4.0, 5.0, 6.0, 4.4, 5.5, 6.6]]], 0.9860135594710389)
unit("correlation_i32", R + "323-336", "CORR", "int32", [[[1, 2, 3], [4, 5, 6]]], 1.0)
unit("correlation_u32", R + "338-350", "CORR", "uint32", [[[1, 2, 3], [4, 5, 6]]], 1.0)
unit("correlation_f32", R + "352-364", "CORR", "float32", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]], 1.0)
unit("correlation_i32_with_nulls_1", R + "366-381", "CORR", "int32", [[[1, N, 3, 3], [4, N, 6, 3]]], 0.1889822365046137)
unit("correlation_i32_with_nulls_2", R + "383-408", "CORR", "int32", [[[1, N, 2, 9, 3], [4, 5, 5, N, 6]]], 1.0)
unit("correlation_i32_all_nulls", R + "410-423", "CORR", "int32", [[[N, N], [N, N]]], N)
unit("correlation_f64_merge_1", R + "425-458", "CORR", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [[1.1, 2.2, 3.3], [4.4, 5.5, 9.9]]], 0.8443707186481967, merge=True)
unit("correlation_f64_merge_2", R + "460-494", "CORR", "float64", [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [[N], [N]]], 1.0, merge=True)

A = "datafusion/sqllogictest/test_files/aggregate.slt:"
COVARS = ["COVAR_SAMP", "COVAR_POP"]
REGR = ["REGR_SLOPE", "REGR_INTERCEPT", "REGR_COUNT", "REGR_R2", "REGR_AVGX", "REGR_AVGY", "REGR_SXX", "REGR_SYY", "REGR_SXY"]
WITH_NULLS = ([1, N, 2, 98, 3, N], [4, 99, 5, N, 6, N])
slt("single_row_query_covar_1", A + "264-268", "float64", [1.1], [2.2], ["COVAR_SAMP"], "NULL")
slt("single_row_query_covar_2", A + "270-274", "float64", [1.1], [2.2], ["COVAR_POP"], "0")
slt("all_nulls_query_covar", A + "276-286", "int32", [N, N], [N, N], COVARS, "NULL NULL")
slt("covar_query_with_nulls", A + "288-306", "int64", *WITH_NULLS, COVARS, "1 0.666666666667")
slt("single_row_query_correlation", A + "314-318", "float64", [1.1], [2.2], ["CORR"], "0")
slt("all_nulls_query_correlation", A + "320-330", "int32", [N, N], [N, N], ["CORR"], "NULL")
slt("correlation_query_with_nulls", A + "332-350", "int64", *WITH_NULLS, ["CORR"], "1")
# regr_*(y, x): argument 0 is y.  The queries over `values` call regr_*(column2, column1): a = column2, b = column1
slt("regr_null_results_1_1", A + "2805-2809", "int64", [1], [1], REGR, "NULL NULL 1 NULL 1 1 0 0 0")
slt("regr_null_results_1_null", A + "2811-2814", "int64", [1], [N], REGR, "NULL NULL 0 NULL NULL NULL NULL NULL NULL")
slt("regr_null_results_null_1", A + "2816-2819", "int64", [N], [1], REGR, "NULL NULL 0 NULL NULL NULL NULL NULL NULL")
slt("regr_null_results_null_null", A + "2821-2824", "int64", [N], [N], REGR, "NULL NULL 0 NULL NULL NULL NULL NULL NULL")
slt("regr_constant_x", A + "2826-2829", "int64", [2, 4, 6], [1, 1, 1], REGR, "NULL NULL 3 NULL 1 4 0 8 0")
slt("regr_basic", A + "2833-2847", "int64", [2, 4, 6], [1, 2, 3], REGR, "2 0 3 1 2 4 2 8 4")
slt("regr_ignore_nulls_1", A + "2866-2880", "int64", [N, 4, 6], [1, 2, 3], REGR, "2 0 2 1 2.5 5 0.5 2 1")
slt("regr_ignore_nulls_2", A + "2882-2895", "int64", [N, 4, 6], [1, N, 3], REGR, "NULL NULL 1 NULL 3 6 0 0 0")
slt("regr_ignore_nulls_3", A + "2897-2910", "int64", [N, 4, N], [1, N, N], REGR, "NULL NULL 0 NULL NULL NULL NULL NULL NULL")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "comoments.json"), "w", encoding="utf-8") as f:
    json.dump({"cases": cases}, f, indent=1)
    f.write("\n")
