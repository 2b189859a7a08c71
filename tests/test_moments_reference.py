"""CPU: the plain-Python model of VarianceAccumulator / StddevAccumulator (tests/moments_reference.py) against the reference's own known answers
(tests/golden/moments.json) and against exact rational arithmetic on the random inputs of tests/test_variance_stddev.py; the C ABI of the device accumulator."""
import ctypes as C
import os
import subprocess

import pytest

import moments_reference as mr
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_golden("moments.json")["cases"]
MOMENT_SYMBOLS = ["dfgpu_moments_evaluate", "dfgpu_moments_free", "dfgpu_moments_merge_batch", "dfgpu_moments_new", "dfgpu_moments_size", "dfgpu_moments_state", "dfgpu_moments_update_batch"]


def slt_text(v):
    """a Float64 cell as sqllogictest prints it: NULL, or rounded to 12 decimals without trailing zeros"""
    if v is None:
        return "NULL"
    s = f"{v:.12f}".rstrip("0").rstrip(".")
    return "0" if s in ("-0", "") else s


def model_answer(case, kind):
    if "values" in case:                                      # .slt: one batch, no GROUP BY
        a = mr.VarianceAccumulator(); a.update_batch(case["values"], case["dtype"])
        return a.evaluate(kind)
    accs = []
    for b in case["batches"]:
        if not accs or case["merge"]:
            accs.append(mr.VarianceAccumulator())
        accs[-1].update_batch(b, case["dtype"])
    for other in accs[1:]:                                    # variance.rs:509-539
        c, m, q = other.state()
        accs[0].merge_batch([c], [m], [q])
    return accs[0].evaluate(kind)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_reference_answers(case):
    """(a) the same IEEE operations as the Rust code: equal with ==, NULLs included"""
    if "values" in case:
        assert [slt_text(model_answer(case, k)) for k in case["kinds"]] == case["expected_text"], case["ref"]
    else:
        got = model_answer(case, case["kind"])
        assert got == case["expected"] and (got is None) == (case["expected"] is None), case["ref"]


def test_golden_file_is_what_the_transcription_writes(tmp_path):
    import json
    import runpy
    import shutil
    shutil.copy(os.path.join(ROOT, "tests", "golden", "transcribe_moments.py"), tmp_path / "transcribe_moments.py")
    runpy.run_path(str(tmp_path / "transcribe_moments.py"))           # writes beside itself
    assert json.load(open(tmp_path / "moments.json")) == load_golden("moments.json")
    assert len(CASES) == 27 and all(":" in c["ref"] for c in CASES)


def model_error(batches, kinds=mr.KINDS, dtype="float64"):
    """the model's largest relative error against exact arithmetic over the groups and kinds of a series of update batches"""
    m = mr.GroupedMoments(dtype=dtype)
    for b in batches:
        m.update_batch(b["values"], b["gids"], b["filter"], b["total"])
    worst = 0.0
    xs = mr.group_values(batches, dtype)
    for kind in kinds:
        for got, x in zip(m.evaluate(kind), xs):
            want = mr.exact_evaluate(kind, x)
            assert (got is None) == (want is None)
            if got is not None:
                worst = max(worst, mr.rel_err(got, want))
    for c, mean, m2, x in zip(*m.state(), xs):
        n, em, eq = mr.exact_state(x)
        assert c == n
        if n:
            scale = max(abs(float(v)) for v in x)
            assert abs(mean - float(em)) <= 1e-9 * max(abs(float(em)), scale) and abs(m2 - float(eq)) <= 1e-9 * max(float(eq), scale * scale)
    return worst


def test_model_meets_the_tolerance_on_the_device_tests_inputs():
    """(b) the yardstick itself is within 1e-9 relative of exact rational arithmetic on every random input the device tests use"""
    for n in mr.PATH_ROWS:
        for total in mr.PATH_TOTALS:
            assert model_error([mr.path_batch(n, total)], kinds=("VAR_SAMP", "STDDEV_POP")) <= 1e-9, (n, total)
    for ids in ("equal", "alternating"):
        for total in (9, mr.MOMENTS_LDS_GROUPS + 1):
            assert model_error([mr.path_batch(4097, total, ids)]) <= 1e-9
    for b in (mr.nulls_filters_batch(), mr.nulls_filters_batch(n=1300, total=29, seed=61), mr.nulls_filters_batch(n=1300, total=29, seed=127)):
        assert max(len(x) for x in mr.group_values([b])) <= 5000
        assert model_error([b]) <= 1e-9
    assert model_error(mr.three_batches()) <= 1e-9
    assert model_error(mr.merge_inputs()) <= 1e-9
    for dtype in ("int8", "int32", "int64", "uint64", "float32", "float64"):
        assert model_error([mr.typed_batch(dtype)], dtype=dtype) <= 1e-9, dtype
    tables = mr.plan_tables()
    ids, _ = mr.first_seen_ids([k for t in tables for k in t["k"]])
    x = [v for t in tables for v in t["x"]]
    assert model_error([mr.batch(x, ids, max(ids) + 1)]) <= 1e-9
    assert model_error([mr.batch(x, ids, max(ids) + 1, [f for t in tables for f in t["f"]])]) <= 1e-9
    tables = mr.plan_tables(seed=6, batches=2, rows=700)
    x = [v for t in tables for v in t["x"]]
    assert model_error([mr.batch(x, [0] * len(x), 1)]) <= 1e-9 and model_error([mr.batch(x, [0] * len(x), 1, [f for t in tables for f in t["f"]])]) <= 1e-9


def test_library_exports_and_binds_the_moments_entry_points():
    """(c) libdfgpu.so exports the seven dfgpu_moments_* symbols and nothing else new, capi.PROTOTYPES binds them, and a NULL context is refused before the device is touched"""
    import dfgpu
    if not os.path.exists(dfgpu.capi.LIB_PATH):
        subprocess.check_call(["make", "-j8", "-C", os.path.join(ROOT, "datafusion-upstream_amd", "csrc")])
    out = subprocess.check_output(["nm", "-D", "--defined-only", dfgpu.capi.LIB_PATH], text=True)
    exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("dfgpu_moments"))
    assert exported == MOMENT_SYMBOLS
    assert sorted(n for n in dfgpu.capi.PROTOTYPES if n.startswith("dfgpu_moments")) == MOMENT_SYMBOLS
    lib = dfgpu.load_library()
    h = C.c_void_p()
    assert lib.dfgpu_moments_new(None, dfgpu.capi.AGG_VAR_SAMP, dfgpu.capi.FLOAT64, C.byref(h)) == 5 and not h.value
    assert (dfgpu.capi.AGG_VAR_SAMP, dfgpu.capi.AGG_VAR_POP, dfgpu.capi.AGG_STDDEV_SAMP, dfgpu.capi.AGG_STDDEV_POP) == (6, 7, 8, 9)
    lib.dfgpu_moments_free(None)
    assert lib.dfgpu_moments_size(None) == 0
    from dfgpu import physical_plan as ops
    names = {"VAR_SAMP": 6, "VAR": 6, "VARIANCE": 6, "VAR_POP": 7, "STDDEV_SAMP": 8, "STDDEV": 8, "STDDEV_POP": 9}
    assert {n: ops.AggregateFunctionExpr(n.lower(), None, "a").kind for n in names} == names
