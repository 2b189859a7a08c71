"""CPU: the plain-Python model of CovarianceAccumulator / CorrelationAccumulator / RegrAccumulator (tests/comoments_reference.py) against the reference's own known answers
(tests/golden/comoments.json) and against exact rational arithmetic on the random inputs of tests/test_two_argument_aggregates.py; the C ABI of the device accumulator and of the
plan layer's second argument."""
import ctypes as C
import math
import os
import subprocess

import pytest

import comoments_reference as cr
from helpers import load_golden
from test_moments_reference import slt_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_golden("comoments.json")["cases"]
COMOMENT_SYMBOLS = ["dfgpu_comoments_evaluate", "dfgpu_comoments_free", "dfgpu_comoments_merge_batch", "dfgpu_comoments_new", "dfgpu_comoments_size", "dfgpu_comoments_state",
                    "dfgpu_comoments_update_batch"]


def model_answer(case, kind):
    new = cr.ACCUMULATORS[cr.family(kind)]
    if "a" in case:                                           # .slt: one batch, no GROUP BY
        acc = new(); acc.update_batch(case["a"], case["b"], case["dtypes"])
        return acc.evaluate(kind)
    accs = []
    for a, b in case["batches"]:
        if not accs or case["merge"]:
            accs.append(new())
        accs[-1].update_batch(a, b, case["dtypes"])
    for other in accs[1:]:                                    # covariance.rs:744-765
        accs[0].merge_batch(*[[s] for s in other.state()])
    return accs[0].evaluate(kind)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_reference_answers(case):
    """(a) the same IEEE operations as the Rust code: every unit-test answer with ==, NULLs included, every .slt cell as the file prints it"""
    if "a" in case:
        assert len(case["kinds"]) == len(case["expected_text"])
        assert [slt_text(model_answer(case, k)) for k in case["kinds"]] == case["expected_text"], case["ref"]
    else:
        got = model_answer(case, case["kind"])
        assert got == case["expected"] and (got is None) == (case["expected"] is None), case["ref"]


def test_golden_file_is_what_the_transcription_writes(tmp_path):
    import json
    import runpy
    import shutil
    shutil.copy(os.path.join(ROOT, "tests", "golden", "transcribe_comoments.py"), tmp_path / "transcribe_comoments.py")
    runpy.run_path(str(tmp_path / "transcribe_comoments.py"))         # writes beside itself
    assert json.load(open(tmp_path / "comoments.json")) == load_golden("comoments.json")
    assert len(CASES) == 45 and all(":" in c["ref"] for c in CASES)
    assert {k for c in CASES for k in (c["kinds"] if "kinds" in c else [c["kind"]])} == set(cr.KINDS)


def check_model_against_exact(batches, kinds=cr.KINDS, dtypes=("float64", "float64")):
    """the model against exact arithmetic over the groups and kinds of a series of update batches, within the tolerance the device tests allow the device against the model
    (1e-9 relative with value_floor / state_floors); NULL exactly where the exact answer is NULL"""
    pairs = cr.group_pairs(batches, dtypes)
    sa, sb = cr.scales(batches, dtypes)
    models = {f: cr.model_of(k, batches, dtypes) for f, k in (("COVAR", "COVAR_POP"), ("CORR", "CORR"), ("REGR", "REGR_SXY")) if any(cr.family(x) == f for x in kinds)}
    for kind in kinds:
        floor = cr.value_floor(kind, sa, sb)
        for g, (got, p) in enumerate(zip(models[cr.family(kind)].evaluate(kind), pairs)):
            want = cr.exact_evaluate(kind, p)
            assert (got is None) == (want is None), (kind, g, got, want)
            if got is not None:
                assert cr.close(got, float(want), floor), (kind, g, got, float(want))
    for fam, m in models.items():
        cols, floors = m.state(), cr.state_floors(fam, sa, sb)
        for g, p in enumerate(pairs):
            n, mean_a, mean_b, m2_a, m2_b, c_ab = cr.exact_state(p)
            exact = {"count": n, "mean1": mean_a, "mean2": mean_b, "m2_1": m2_a, "m2_2": m2_b, "mean_x": mean_b, "mean_y": mean_a, "m2_x": m2_b, "m2_y": m2_a, "algo_const": c_ab}
            assert cols[0][g] == n
            for name, col, floor in zip(cr.STATE_NAMES[fam][1:], cols[1:], floors[1:]):
                assert cr.close(col[g], float(exact[name]), floor), (fam, name, g, col[g], float(exact[name]))


def test_model_meets_the_tolerance_on_the_device_tests_inputs():
    """(b) the yardstick itself is within the device tests' tolerance of exact rational arithmetic on every random input they use: this is what licenses that tolerance"""
    for n in cr.PATH_ROWS:
        for total in cr.PATH_TOTALS:
            check_model_against_exact([cr.path_batch(n, total)])
    for total in cr.PATH_TOTALS:
        check_model_against_exact(cr.ragged_batches(total))
    for ids in ("equal", "alternating"):
        for total in (9, cr.COMOMENTS_LDS_SMALL + 9, cr.COMOMENTS_LDS_GROUPS + 1):
            check_model_against_exact([cr.path_batch(4097, total, ids)], kinds=("COVAR_SAMP", "CORR", "REGR_SLOPE", "REGR_INTERCEPT", "REGR_R2"))
    for b in (cr.nulls_filters_batch(), cr.nulls_filters_batch(n=1300, total=29, seed=61, all_null_group=False), cr.nulls_filters_batch(n=1300, total=29, seed=124, all_null_group=False),
              cr.nulls_filters_batch(n=1300, total=29, seed=125, all_null_group=False)):
        check_model_against_exact([b])
    check_model_against_exact(cr.growing_batches())
    check_model_against_exact(cr.merge_inputs())
    tables = cr.plan_tables()
    ids, _ = cr.first_seen_ids([k for t in tables for k in t["k"]])
    y, x, f = [v for t in tables for v in t["y"]], [v for t in tables for v in t["x"]], [v for t in tables for v in t["f"]]
    check_model_against_exact([cr.batch(y, x, ids, max(ids) + 1)])
    check_model_against_exact([cr.batch(y, x, ids, max(ids) + 1, f)], kinds=("COVAR_SAMP",))
    v = [w for t in tables for w in t["v"]]
    check_model_against_exact([cr.batch(v, x, ids, max(ids) + 1)], kinds=("CORR",), dtypes=("int32", "float64"))
    check_model_against_exact([cr.batch(y, v, ids, max(ids) + 1, f)], kinds=("REGR_SLOPE",), dtypes=("float64", "int32"))
    tables = cr.plan_tables(seed=8, batches=2, rows=1500, groups=12)                  # below FilterExec(w > -5)
    keep = [i for i, w in enumerate(w for t in tables for w in t["w"]) if w > -5.0]
    col = {c: [v for t in tables for v in t[c]] for c in ("k", "y", "x", "v", "f")}
    ids, _ = cr.first_seen_ids([col["k"][i] for i in keep])
    pick = lambda c: [col[c][i] for i in keep]
    check_model_against_exact([cr.batch(pick("y"), pick("x"), ids, max(ids) + 1)])
    check_model_against_exact([cr.batch(pick("y"), pick("x"), ids, max(ids) + 1, pick("f"))], kinds=("COVAR_SAMP",))
    check_model_against_exact([cr.batch(pick("v"), pick("x"), ids, max(ids) + 1)], kinds=("CORR",), dtypes=("int32", "float64"))
    check_model_against_exact([cr.batch(pick("y"), pick("v"), ids, max(ids) + 1, pick("f"))], kinds=("REGR_SLOPE",), dtypes=("float64", "int32"))
    check_model_against_exact([cr.batch(pick("y"), pick("x"), [0] * len(keep), 1)], kinds=("CORR", "COVAR_POP"))
    tables = cr.plan_tables(seed=6, batches=2, rows=700)
    y, x = [v for t in tables for v in t["y"]], [v for t in tables for v in t["x"]]
    check_model_against_exact([cr.batch(y, x, [0] * len(y), 1)])


def test_model_on_mixed_types_meets_the_tolerance():
    """each argument cast `as f64` on its own: Int32 x Float64, UInt64 x Float32, Int8 x Int8 over their whole ranges"""
    for dtypes in cr.TYPE_PAIRS:
        b = cr.typed_batch(dtypes)
        if dtypes[0] == "uint64":
            assert max(b["a"]) > 2 ** 63
        check_model_against_exact([b], dtypes=dtypes)


@pytest.mark.parametrize("total", [4, cr.COMOMENTS_LDS_GROUPS + 1])
def test_model_keeps_exact_zeros_for_a_constant_argument(total):
    """the property the device must reproduce: 0.1 in every row of a group keeps that argument's m2 and the group's algo_const at exactly 0.0 in the reference's
    recurrences, so CORR is 0.0 and SLOPE / INTERCEPT / R2 are NULL where x is the constant; and a sum-then-divide mean does NOT give 0.1 back for these counts"""
    batches = cr.constant_batches(total)
    assert len(batches) >= 3 and all(len(b["gids"]) > 64 for b in batches)
    corr, regr = cr.model_of("CORR", batches), cr.model_of("REGR_SLOPE", batches)
    assert corr.evaluate()[:3] == [0.0, 0.0, 0.0] and all(v != 0.0 for v in corr.evaluate()[3:])
    for g, (sxx_zero, syy_zero) in enumerate([(False, True), (True, False), (True, True)]):          # a = y, b = x
        _, _, _, m2_x, m2_y, c = regr.accs[g].state()
        assert (m2_x == 0.0, m2_y == 0.0, c == 0.0) == (sxx_zero, syy_zero, True)
        assert (regr.evaluate("REGR_SLOPE")[g] is None, regr.evaluate("REGR_R2")[g] is None) == (sxx_zero, True)
    assert regr.evaluate("REGR_SLOPE")[0] == 0.0 and all(v is not None for k in cr.REGR_KINDS for v in regr.evaluate(k)[3:])
    n = corr.accs[0].covar.count
    assert n > 192 and math.fsum([cr.CONSTANT] * n) / n == cr.CONSTANT          # exactly rounded sums would be fine; the device's are not exactly rounded:
    s = 0.0
    for _ in range(n):
        s += cr.CONSTANT
    assert s / n != cr.CONSTANT


def test_library_exports_and_binds_the_comoments_entry_points():
    """(c) libdfgpu.so exports the seven dfgpu_comoments_* symbols and dfgpu_plan_aggregate_second_arg, capi.PROTOTYPES binds them, NULL handles are refused before the device
    is touched, and the Python plan builders know the names BuiltinAggregateFunction::from_str accepts"""
    import dfgpu
    if not os.path.exists(dfgpu.capi.LIB_PATH):
        subprocess.check_call(["make", "-j8", "-C", os.path.join(ROOT, "datafusion-upstream_amd", "csrc")])
    out = subprocess.check_output(["nm", "-D", "--defined-only", dfgpu.capi.LIB_PATH], text=True)
    exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("dfgpu_comoments"))
    assert exported == COMOMENT_SYMBOLS
    assert sorted(n for n in dfgpu.capi.PROTOTYPES if n.startswith("dfgpu_comoments")) == COMOMENT_SYMBOLS and "dfgpu_plan_aggregate_second_arg" in dfgpu.capi.PROTOTYPES
    lib = dfgpu.load_library()
    h = C.c_void_p()
    assert lib.dfgpu_comoments_new(None, dfgpu.capi.AGG_CORR, dfgpu.capi.FLOAT64, dfgpu.capi.INT32, C.byref(h)) == 5 and not h.value
    assert lib.dfgpu_comoments_update_batch(None, None, None, None, None, None, 0) == 5 and lib.dfgpu_comoments_merge_batch(None, None, None, 0, None, None, 0) == 5
    assert lib.dfgpu_comoments_state(None, None, None) == 5 and lib.dfgpu_comoments_evaluate(None, None, None) == 5
    assert lib.dfgpu_plan_aggregate_second_arg(None, 0, None, None) == 5
    lib.dfgpu_comoments_free(None)
    assert lib.dfgpu_comoments_size(None) == 0
    assert {k: getattr(dfgpu.capi, "AGG_" + k) for k in cr.KINDS} == cr.KIND_CODES and sorted(cr.KIND_CODES.values()) == list(range(11, 23))
    from dfgpu import physical_plan as ops
    names = dict(cr.KIND_CODES, COVAR=cr.KIND_CODES["COVAR_SAMP"])
    assert {n: ops.AggregateFunctionExpr(n.lower(), None, "a").kind for n in names} == names
    e = ops.AggregateFunctionExpr("corr", None, "a")
    assert e.expr2 is None and e.input_field2 is None and dfgpu.CoMomentsAccumulator is not None
    src = open(os.path.join(ROOT, "datafusion-upstream_amd", "csrc", "comoments.hip")).read()
    assert [int(src.split(f"constexpr int {n} = ")[1].split(";")[0]) for n in ("COMOMENTS_LDS_GROUPS", "COMOMENTS_LDS_SMALL")] == [cr.COMOMENTS_LDS_GROUPS, cr.COMOMENTS_LDS_SMALL]
