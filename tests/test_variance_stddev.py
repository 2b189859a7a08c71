"""-m gpu: VAR_SAMP / VAR_POP / STDDEV_SAMP / STDDEV_POP on the device -- the kernel accumulator (csrc/moments.hip through dfgpu.MomentsAccumulator) and AggregateExec --
against the plain-Python model of the reference's VarianceAccumulator (tests/moments_reference.py; tests/test_moments_reference.py pins the model on the reference's known
answers and shows that it is within 1e-9 of exact arithmetic on these inputs).  Results and state mean / m2: 1e-9 relative (mean and m2 with an absolute floor of 1e-9 x the
largest |value| / |value|^2, both can be near 0); NULL-ness, counts and the 0.0 / NULL at count 1: exact."""
import math

import numpy as np
import pyarrow as pa
import pytest

import moments_reference as mr
from helpers import load_golden

T = 1024                    # MOMENTS_LDS_GROUPS of csrc/moments.hip: up to T groups take the LDS path, T + 1 the global one
assert T == mr.MOMENTS_LDS_GROUPS
PA = {"int8": pa.int8(), "int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64(), "uint8": pa.uint8(), "uint16": pa.uint16(), "uint32": pa.uint32(), "uint64": pa.uint64(),
      "float32": pa.float32(), "float64": pa.float64()}
CASES = load_golden("moments.json")["cases"]


def code(dtype):
    from dfgpu import capi
    return getattr(capi, dtype.upper())


def new_acc(ctx, kind, dtype="float64"):
    import dfgpu
    return dfgpu.MomentsAccumulator(ctx, getattr(dfgpu.capi, "AGG_" + kind), code(dtype))


def dev_ids(ctx, gids):
    return ctx.from_arrow(pa.array(np.asarray(gids, dtype=np.uint32)))


def dev_update(ctx, acc, b, dtype="float64"):
    f = b["filter"]
    acc.update_batch(ctx.from_arrow(pa.array(b["values"], type=PA[dtype])), dev_ids(ctx, b["gids"]), None if f is None else ctx.from_arrow(pa.array(f, type=pa.bool_())), b["total"])


def model_of(kind, batches, dtype="float64"):
    m = mr.GroupedMoments(kind, dtype)
    for b in batches:
        m.update_batch(b["values"], b["gids"], b["filter"], b["total"])
    return m


def close(got, want, floor=0.0):
    return abs(got - want) <= max(1e-9 * abs(want), floor)


def check_values(got, want):
    """evaluate(): NULL exactly where the model is NULL, NaN exactly where it is NaN, a count-1 answer exactly 0.0, else 1e-9 relative"""
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (g, a, b)
        if b is None:
            continue
        if math.isnan(b) or math.isnan(a):
            assert math.isnan(a) and math.isnan(b), (g, a, b)
        else:
            assert close(a, b), (g, a, b)


def check_state(acc, model, scale):
    c, mean, m2 = [s.to_arrow() for s in acc.state()]
    assert (c.type, mean.type, m2.type) == (pa.uint64(), pa.float64(), pa.float64()) and c.null_count == mean.null_count == m2.null_count == 0
    mc, mm, mq = model.state()
    assert c.to_pylist() == mc
    for g, (a, b) in enumerate(zip(mean.to_pylist(), mm)):
        assert close(a, b, 1e-9 * scale), ("mean", g, a, b)
    for g, (a, b) in enumerate(zip(m2.to_pylist(), mq)):
        assert close(a, b, 1e-9 * scale * scale), ("m2", g, a, b)


def largest(batches, dtype="float64"):
    return max([abs(mr.as_f64(v, dtype)) for b in batches for v in b["values"] if v is not None] + [0.0])


def check_against_model(ctx, kind, batches, dtype="float64"):
    acc = new_acc(ctx, kind, dtype)
    for b in batches:
        dev_update(ctx, acc, b, dtype)
    model = model_of(kind, batches, dtype)
    for b in batches[-1:]:
        assert len(model.accs) == b["total"]
    check_values(acc.evaluate().to_arrow().to_pylist(), model.evaluate())
    check_state(acc, model, largest(batches, dtype))
    assert acc.size() >= 24 * len(model.accs)
    return acc, model


# ------------------------------------------------------------------ 1. the reference's known answers, all four kinds
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_answers(ctx, case):
    dtype = case["dtype"]
    if "values" in case:                              # .slt: every output column of the query
        for kind, text in zip(case["kinds"], case["expected_text"]):
            acc = new_acc(ctx, kind, dtype)
            dev_update(ctx, acc, mr.batch(case["values"], [0] * len(case["values"]), 1), dtype)
            got = acc.evaluate().to_arrow().to_pylist()
            assert len(got) == 1 and ((got[0] is None) if text == "NULL" else close(got[0], float(text), 0.5e-12)), (case["ref"], kind, got)       # the file prints 12 decimals
        return
    accs = []
    for b in case["batches"]:
        if not accs or case["merge"]:
            accs.append(new_acc(ctx, case["kind"], dtype))
        dev_update(ctx, accs[-1], mr.batch(b, [0] * len(b), 1), dtype)
    for other in accs[1:]:
        accs[0].merge_batch(other.state(), dev_ids(ctx, [0]), None, 1)
    got, want = accs[0].evaluate().to_arrow().to_pylist(), case["expected"]
    assert len(got) == 1 and ((got[0] is None) if want is None else (got[0] is not None and close(got[0], want))), (case["ref"], got, want)


# ------------------------------------------------------------------ 2. both paths, ragged sizes
@pytest.mark.gpu
@pytest.mark.parametrize("total", mr.PATH_TOTALS)
@pytest.mark.parametrize("n", mr.PATH_ROWS)
def test_paths_and_sizes(ctx, n, total):
    kind = mr.KINDS[(mr.PATH_ROWS.index(n) + mr.PATH_TOTALS.index(total)) % 4]
    check_against_model(ctx, kind, [mr.path_batch(n, total)])


@pytest.mark.gpu
@pytest.mark.parametrize("total", [9, T + 1])
@pytest.mark.parametrize("ids", ["equal", "alternating"])
def test_wave_uniform_and_never_uniform_ids(ctx, ids, total):
    """all-equal ids: every wave takes the one-add-per-wave shortcut; strictly alternating ids: no wave does -- on the LDS and on the global path"""
    for kind in ("VAR_POP", "STDDEV_SAMP"):
        check_against_model(ctx, kind, [mr.path_batch(4097, total, ids)])


# ------------------------------------------------------------------ 3. NULLs, filters, skipped ids, array views
@pytest.mark.gpu
def test_nulls_filters_and_skipped_ids(ctx):
    b = mr.nulls_filters_batch()
    assert any(v is None for v in b["values"]) and {True, False, None} <= set(b["filter"]) and mr.GID_NONE in b["gids"]
    for kind in mr.KINDS:
        check_against_model(ctx, kind, [b])


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1, 67])
def test_values_ids_and_filter_as_slices(ctx, offset):
    """values, ids and filter are views that start `offset` rows into longer arrays: the validity and filter bitmaps start inside a 64-bit word"""
    b = mr.nulls_filters_batch(n=1300, total=29, seed=60 + offset)
    n = len(b["gids"])
    pad_v, pad_g, pad_f = [123.5, None] * 40, [3, mr.GID_NONE] * 40, [True, None] * 40
    v = ctx.from_arrow(pa.array(pad_v[:offset] + b["values"] + pad_v[:9], type=pa.float64())).slice(offset, n)
    g = dev_ids(ctx, pad_g[:offset] + b["gids"] + pad_g[:9]).slice(offset, n)
    f = ctx.from_arrow(pa.array(pad_f[:offset] + b["filter"] + pad_f[:9], type=pa.bool_())).slice(offset, n)
    acc = new_acc(ctx, "VAR_SAMP")
    acc.update_batch(v, g, f, b["total"])
    model = model_of("VAR_SAMP", [b])
    check_values(acc.evaluate().to_arrow().to_pylist(), model.evaluate())
    check_state(acc, model, largest([b]))


# ------------------------------------------------------------------ 4. input types
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "int32", "int64", "uint64", "float32", "float64"])
def test_input_types_are_cast_as_f64(ctx, dtype):
    b = mr.typed_batch(dtype)
    if dtype == "uint64":
        assert max(b["values"]) > 2 ** 63
    check_against_model(ctx, "VAR_SAMP", [b], dtype)
    check_against_model(ctx, "STDDEV_POP", [b], dtype)


@pytest.mark.gpu
def test_other_input_types_and_kinds_are_refused(ctx):
    import dfgpu
    for t in (dfgpu.capi.DECIMAL128, dfgpu.capi.UTF8):
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.MomentsAccumulator(ctx, dfgpu.capi.AGG_VAR_SAMP, t)
        assert e.value.kind == "NotImplemented"
    for kind in (dfgpu.capi.AGG_SUM, 5, 10):
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.MomentsAccumulator(ctx, kind, dfgpu.capi.FLOAT64)
        assert e.value.kind == "InvalidArgument"
    for kind in (6, 7, 8, 9):                                   # dfgpu_acc keeps answering what it answered before these kinds existed
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.GroupsAccumulator(ctx, kind, dfgpu.capi.FLOAT64)
        assert e.value.kind == "InvalidArgument" and f"unknown aggregate kind {kind}" in str(e.value)


# ------------------------------------------------------------------ 5. several batches, growing state
@pytest.mark.gpu
def test_three_batches_with_new_groups(ctx):
    batches = mr.three_batches()
    assert batches[0]["total"] < batches[1]["total"] <= T < batches[2]["total"]
    acc, model = check_against_model(ctx, "STDDEV_SAMP", batches)
    acc.update_batch(None, dev_ids(ctx, []), None, batches[2]["total"] + 5)          # a zero-row update grows the state
    assert acc.state()[0].to_arrow().to_pylist() == model.state()[0] + [0] * 5 and acc.evaluate().to_arrow().to_pylist()[-5:] == [None] * 5


# ------------------------------------------------------------------ 6. merge
def dev_states(ctx, states):
    c, m, q = states
    return [ctx.from_arrow(pa.array(c, type=pa.uint64())), ctx.from_arrow(pa.array(m, type=pa.float64())), ctx.from_arrow(pa.array(q, type=pa.float64()))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["VAR_SAMP", "STDDEV_POP"])
def test_merge_two_accumulators_into_a_third(ctx, kind):
    """every group appears twice in ONE merge_batch call (a Final stage sees a partial row per input partition); rows with count 0 take no part"""
    inputs = mr.merge_inputs()
    total = inputs[0]["total"]
    parts = []
    for b in inputs:
        a = new_acc(ctx, kind); dev_update(ctx, a, b); parts.append(a)
    st = [[x.to_arrow() for x in a.state()] for a in parts]
    empties = (pa.array([0, 0], type=pa.uint64()), pa.array([5.0, float("nan")]), pa.array([7.0, float("inf")]))          # count 0: skipped whatever mean and m2 say
    cols = [ctx.from_arrow(pa.concat_arrays([st[0][k], empties[k], st[1][k]])) for k in range(3)]
    ids = list(range(total)) + [0, total - 1] + list(range(total))
    third = new_acc(ctx, kind)
    third.merge_batch(cols, dev_ids(ctx, ids), None, total)                        # into an empty accumulator
    model = mr.GroupedMoments(kind)
    pm = [model_of(kind, [b]) for b in inputs]
    model.merge_batch(pm[0].state(), list(range(total)), None, total)
    model.merge_batch(pm[1].state(), list(range(total)), None, total)
    check_values(third.evaluate().to_arrow().to_pylist(), model.evaluate())
    check_state(third, model, largest(inputs))
    direct = model_of(kind, inputs)                                                 # and the merged answer is the answer over all rows
    check_values(third.evaluate().to_arrow().to_pylist(), direct.evaluate())
    # with a filter and skipped ids
    rng = np.random.default_rng(9)
    filt = [[True, False, None][k] for k in rng.integers(0, 3, total)]
    gids = [mr.GID_NONE if r < 0.2 else g for g, r in zip(range(total), rng.random(total))]
    fourth, m4 = new_acc(ctx, kind), mr.GroupedMoments(kind)
    fourth.merge_batch(parts[0].state(), dev_ids(ctx, gids), ctx.from_arrow(pa.array(filt, type=pa.bool_())), total)
    m4.merge_batch(pm[0].state(), gids, filt, total)
    check_values(fourth.evaluate().to_arrow().to_pylist(), m4.evaluate())
    check_state(fourth, m4, largest(inputs))


@pytest.mark.gpu
def test_malformed_states_are_refused_and_nothing_is_merged(ctx):
    import dfgpu
    b = mr.path_batch(255, 9)
    acc = new_acc(ctx, "VAR_POP"); dev_update(ctx, acc, b)
    before = [s.to_arrow() for s in acc.state()]
    good = dev_states(ctx, ([2] * 9, [1.0] * 9, [3.0] * 9))
    ids = dev_ids(ctx, list(range(9)))
    bad = {"two columns": good[:2], "four columns": good + good[:1],
           "Int64 counts": [ctx.from_arrow(pa.array([2] * 9, type=pa.int64()))] + good[1:],
           "Float32 means": [good[0], ctx.from_arrow(pa.array([1.0] * 9, type=pa.float32())), good[2]],
           "UInt64 m2": [good[0], good[1], ctx.from_arrow(pa.array([3] * 9, type=pa.uint64()))],
           "short m2": [good[0], good[1], ctx.from_arrow(pa.array([3.0] * 8, type=pa.float64()))],
           "short counts": [ctx.from_arrow(pa.array([2] * 8, type=pa.uint64()))] + good[1:]}
    for what, st in bad.items():
        with pytest.raises(dfgpu.DfgpuError) as e:
            acc.merge_batch(st, ids, None, 12)
        assert e.value.kind == "InvalidArgument", what
        after = [s.to_arrow() for s in acc.state()]
        assert all(x.equals(y) for x, y in zip(before, after)), what                 # not even grown to 12 groups
    acc.merge_batch(good, ids, None, 12)
    assert acc.state()[0].to_arrow().to_pylist() == [c + 2 for c in before[0].to_pylist()] + [0, 0, 0]


# ------------------------------------------------------------------ 7. an id beyond the groups
@pytest.mark.gpu
@pytest.mark.parametrize("total", [3, T + 5])
def test_group_id_out_of_range_is_the_accumulators_error(ctx, total):
    import dfgpu
    v = ctx.from_arrow(pa.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    g = dev_ids(ctx, [0, 1, total, 2, 1])
    errors = []
    for acc in (dfgpu.GroupsAccumulator(ctx, dfgpu.capi.AGG_MAX, dfgpu.capi.FLOAT64), new_acc(ctx, "VAR_SAMP")):
        with pytest.raises(dfgpu.DfgpuError) as e:
            acc.update_batch(v, g, None, total)
        errors.append(e.value)
    assert errors[0].kind == errors[1].kind == "Execution"
    assert "Arrow error: index out of bounds" in str(errors[0]) and "Arrow error: index out of bounds" in str(errors[1])
    acc = new_acc(ctx, "VAR_SAMP")
    with pytest.raises(dfgpu.DfgpuError) as e:
        acc.merge_batch(dev_states(ctx, ([1] * 5, [1.0] * 5, [0.0] * 5)), g, None, total)
    assert e.value.kind == "Execution" and "index out of bounds" in str(e.value)


# ------------------------------------------------------------------ 8. NaN and infinity
@pytest.mark.gpu
@pytest.mark.parametrize("total", [4, T + 1])
def test_nan_and_infinity(ctx, total):
    """group 0 holds a NaN, group 1 +Inf among finite values, group 2 only finite values, group 3 +Inf alone: NaN exactly where the model's answer is NaN"""
    values = [1.0, float("nan"), 2.0, 5.0, float("inf"), 7.0, 1.5, 2.5, 4.0, float("inf")]
    gids = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    b = mr.batch(values, gids, total)
    for kind in mr.KINDS:
        acc = new_acc(ctx, kind); dev_update(ctx, acc, b)
        want = model_of(kind, [b]).evaluate()
        assert math.isnan(want[0]) and math.isnan(want[1]) and not math.isnan(want[2])
        check_values(acc.evaluate().to_arrow().to_pylist(), want)


# ------------------------------------------------------------------ 9. ill-conditioned input
@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 7])
def test_ill_conditioned_against_exact_arithmetic(ctx, groups):
    """4096 rows of 1e9 + k % 7 (mean / sd = 5e8): the device's relative error against exact rational arithmetic is at most max(1e-9, the model's own error) --
    the yardstick is what the reference's recurrence loses on the same input, not what the code under test gives"""
    b = mr.ill_conditioned(groups)
    xs = mr.group_values([b])
    for kind in ("VAR_SAMP", "STDDEV_POP"):
        acc = new_acc(ctx, kind); dev_update(ctx, acc, b)
        got, model = acc.evaluate().to_arrow().to_pylist(), model_of(kind, [b]).evaluate()
        for g in range(groups):
            exact = mr.exact_evaluate(kind, xs[g])
            dev_err, model_err = mr.rel_err(got[g], exact), mr.rel_err(model[g], exact)
            print(f"ill-conditioned {kind} groups={groups} g={g}: device {dev_err:.3e} model {model_err:.3e}")
            assert dev_err <= max(1e-9, model_err), (kind, g, dev_err, model_err)


# ------------------------------------------------------------------ plan level
def table_of(t):
    return pa.table({"k": pa.array(t["k"], type=pa.int64()), "x": pa.array(t["x"], type=pa.float64()), "f": pa.array(t["f"], type=pa.bool_())})


def agg_plan(ctx, tables, keys, aggs, mode="Single"):
    """the shape of tests/test_plan_aggregates.py agg_plan, with an optional FILTER column per aggregate: aggs = [(fun, column, output name, filter column or None)]"""
    from dfgpu import capi, physical_plan as ops
    bs = [ops.batch_from_arrow(ctx, t) for t in tables]
    src = ops.MemoryExec([bs], bs[0].schema)
    names = tables[0].column_names
    C, F = ops.Column, ops.Field

    def mk(with_filters=True):
        return [ops.AggregateFunctionExpr(fun, C(col, names.index(col)), name, filter=C(flt, names.index(flt)) if flt and with_filters else None, input_field=F(col, capi.FLOAT64))
                for fun, col, name, flt in aggs]
    gb = [(C(k, names.index(k)), k) for k in keys]
    if mode == "Single":
        plan = ops.AggregateExec("Single", gb, mk(), src)
    elif mode == "Partial":
        plan = ops.AggregateExec("Partial", gb, mk(), src)
    else:
        plan = ops.AggregateExec("FinalPartitioned", [(C(k, i), k) for i, k in enumerate(keys)], mk(False), ops.AggregateExec("Partial", gb, mk(), src))
    return pa.concat_tables([b.to_arrow() for b in plan.execute(0, ops.TaskContext(ctx, 8192))])


MOMENT_AGGS = [("VAR_SAMP", "x", "var_samp", None), ("VAR_POP", "x", "var_pop", None), ("STDDEV_SAMP", "x", "stddev_samp", None), ("STDDEV_POP", "x", "stddev_pop", None),
               ("VAR", "x", "var_f", "f")]
PLAIN_AGGS = [("SUM", "x", "sum", None), ("COUNT", "x", "count", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Single", "PartialFinal"])
def test_plan_grouped(ctx, mode):
    """3 batches of 4000 rows, 40 groups and the NULL key group; the four kinds, one of them again under FILTER (WHERE f), SUM and COUNT of the same column beside them.
    x holds multiples of 1/64, so SUM(x) is exact in any order and must EQUAL what the plan without the new aggregates gives."""
    tables = mr.plan_tables()
    pt = [table_of(t) for t in tables]
    out = agg_plan(ctx, pt, ["k"], MOMENT_AGGS + PLAIN_AGGS, mode)
    plain = agg_plan(ctx, pt, ["k"], PLAIN_AGGS, mode)
    keys = [k for t in tables for k in t["k"]]
    ids, table = mr.first_seen_ids(keys)
    total = len(table)
    assert total == 41 and None in table
    assert out["k"].to_pylist() == list(table) == plain["k"].to_pylist()                         # first-seen order
    assert out["sum"].to_pylist() == plain["sum"].to_pylist() and out["count"].to_pylist() == plain["count"].to_pylist()
    x = [v for t in tables for v in t["x"]]
    f = [v for t in tables for v in t["f"]]
    model = model_of("VAR_SAMP", [mr.batch(x, ids, total)])
    for kind, _, name, _ in MOMENT_AGGS[:4]:
        check_values(out[name].to_pylist(), model.evaluate(kind))
    check_values(out["var_f"].to_pylist(), model_of("VAR_SAMP", [mr.batch(x, ids, total, f)]).evaluate())
    assert out["count"].to_pylist() == model.state()[0]
    assert all(c.type == pa.float64() for c in (out[n[2]] for n in MOMENT_AGGS))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Single", "PartialFinal"])
def test_plan_without_group_by(ctx, mode):
    empty = pa.table({"k": pa.array([], type=pa.int64()), "x": pa.array([], type=pa.float64()), "f": pa.array([], type=pa.bool_())})
    out = agg_plan(ctx, [empty], [], MOMENT_AGGS[:4], mode)
    assert out.num_rows == 1 and [out.column(i)[0].as_py() for i in range(4)] == [None, None, None, None]
    one = pa.table({"k": pa.array([1], type=pa.int64()), "x": pa.array([3.5], type=pa.float64()), "f": pa.array([True])})
    out = agg_plan(ctx, [one], [], MOMENT_AGGS[:4], mode)
    got = [out.column(i)[0].as_py() for i in range(4)]
    assert out.num_rows == 1 and got == [None, 0.0, None, 0.0] and math.copysign(1.0, got[1]) == 1.0
    tables = mr.plan_tables(seed=6, batches=2, rows=700)
    out = agg_plan(ctx, [table_of(t) for t in tables], [], MOMENT_AGGS, mode)
    x = [v for t in tables for v in t["x"]]
    f = [v for t in tables for v in t["f"]]
    model = model_of("VAR_SAMP", [mr.batch(x, [0] * len(x), 1)])
    for kind, _, name, _ in MOMENT_AGGS[:4]:
        check_values(out[name].to_pylist(), model.evaluate(kind))
    check_values(out["var_f"].to_pylist(), model_of("VAR_SAMP", [mr.batch(x, [0] * len(x), 1, f)]).evaluate())


@pytest.mark.gpu
def test_partial_stage_schema(ctx):
    """the Partial stage emits name[count] UInt64, name[mean] Float64, name[m2] Float64 per moment aggregate (variance.rs:86-100), without NULLs, also for a group without values"""
    t = pa.table({"k": pa.array([1, 1, 2, 3, 3, 3], type=pa.int64()), "x": pa.array([1.0, 2.0, None, 4.0, 6.0, 8.0]), "f": pa.array([True] * 6)})
    out = agg_plan(ctx, [t], ["k"], [("STDDEV_POP", "x", "x", None), ("SUM", "x", "s", None)], "Partial")
    assert out.column_names == ["k", "x[count]", "x[mean]", "x[m2]", "s[sum]"]
    assert [out.schema.field(i).type for i in (1, 2, 3)] == [pa.uint64(), pa.float64(), pa.float64()]
    assert all(out.column(i).null_count == 0 for i in (1, 2, 3))
    assert out["x[count]"].to_pylist() == [2, 0, 3]
    assert all(close(a, b) for a, b in zip(out["x[mean]"].to_pylist(), [1.5, 0.0, 6.0])) and all(close(a, b) for a, b in zip(out["x[m2]"].to_pylist(), [0.5, 0.0, 8.0]))


@pytest.mark.gpu
def test_grouping_sets_and_unknown_kinds_are_refused(ctx):
    import dfgpu
    from dfgpu import capi, physical_plan as ops
    t = table_of(mr.plan_tables(seed=7, batches=1, rows=50)[0])
    b = ops.batch_from_arrow(ctx, t)
    C, F, L = ops.Column, ops.Field, ops.Literal
    gb = ops.PhysicalGroupBy([(C("k", 0), "k")], [(L(None, pa.int64()), "k")], [[False], [True]])
    tc = ops.TaskContext(ctx, 8192)
    with pytest.raises(dfgpu.DfgpuError) as e:
        list(ops.AggregateExec("Single", gb, [ops.AggregateFunctionExpr("STDDEV", C("x", 1), "sd", input_field=F("x", capi.FLOAT64))], ops.MemoryExec([[b]], b.schema)).execute(0, tc))
    assert e.value.kind == "NotImplemented" and "grouping sets" in str(e.value) and "sd" in str(e.value)
    out = list(ops.AggregateExec("Single", gb, [ops.AggregateFunctionExpr("COUNT", C("x", 1), "n", input_field=F("x", capi.FLOAT64))], ops.MemoryExec([[b]], b.schema)).execute(0, tc))
    assert sum(o.to_arrow().num_rows for o in out) > 1                                  # grouping sets themselves still work

    class Kind10(ops.AggregateFunctionExpr):
        kind = property(lambda self: 10)
    with pytest.raises(dfgpu.DfgpuError) as e:
        list(ops.AggregateExec("Single", [(C("k", 0), "k")], [Kind10("?", C("x", 1), "a", input_field=F("x", capi.FLOAT64))], ops.MemoryExec([[b]], b.schema)).execute(0, tc))
    assert e.value.kind == "NotImplemented" and "aggregate kind 10 has no GroupsAccumulator on device" in str(e.value)
    for typ in (capi.UTF8, capi.DECIMAL128, capi.BOOL, capi.DATE32):
        with pytest.raises(dfgpu.DfgpuError) as e:
            list(ops.AggregateExec("Final", [(C("k", 0), "k")], [ops.AggregateFunctionExpr("VAR_POP", C("x", 1), "a", input_field=F("x", typ, 10, 2))], ops.MemoryExec([[b]], b.schema)).execute(0, tc))
        assert e.value.kind == "NotImplemented" and "kind 7" in str(e.value) and f"type {typ}" in str(e.value)
