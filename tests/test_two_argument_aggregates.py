"""-m gpu: COVAR_SAMP / COVAR_POP / CORR / REGR_SLOPE .. REGR_SXY on the device -- the kernel accumulator (csrc/comoments.hip through dfgpu.CoMomentsAccumulator) and
AggregateExec -- against the plain-Python model of the reference's CovarianceAccumulator / CorrelationAccumulator / RegrAccumulator (tests/comoments_reference.py;
tests/test_comoments_reference.py pins the model on the reference's known answers and shows that it is within this file's tolerance of exact arithmetic on these inputs).
Results and the Float64 state columns: 1e-9 relative, with the absolute floors of comoments_reference.value_floor / state_floors (1e-9 of the quantity's unit built from the
largest |value| of each argument; CORR and R2: 1e-9).  Exact: NULL-ness, counts, REGR_COUNT, the 0.0 of CORR at count 1 and at a constant argument, the NULLs of
SLOPE / INTERCEPT / R2 at a constant x."""
import math

import numpy as np
import pyarrow as pa
import pytest

import comoments_reference as cr
from helpers import load_golden

T = 1024                    # COMOMENTS_LDS_GROUPS of csrc/comoments.hip: up to T groups take the LDS path, T + 1 the global one
S = 512                     # COMOMENTS_LDS_SMALL: up to S groups the LDS path runs with its smaller arrays
assert (T, S) == (cr.COMOMENTS_LDS_GROUPS, cr.COMOMENTS_LDS_SMALL)
PA = {"int8": pa.int8(), "int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64(), "uint8": pa.uint8(), "uint16": pa.uint16(), "uint32": pa.uint32(), "uint64": pa.uint64(),
      "float32": pa.float32(), "float64": pa.float64()}
F64 = ("float64", "float64")
CASES = load_golden("comoments.json")["cases"]
ONE_PER_FAMILY = ("COVAR_SAMP", "CORR", "REGR_INTERCEPT")


def code(dtype):
    from dfgpu import capi
    return getattr(capi, dtype.upper())


def new_acc(ctx, kind, dtypes=F64):
    import dfgpu
    assert getattr(dfgpu.capi, "AGG_" + kind) == cr.KIND_CODES[kind]
    return dfgpu.CoMomentsAccumulator(ctx, cr.KIND_CODES[kind], code(dtypes[0]), code(dtypes[1]))


def dev_ids(ctx, gids):
    return ctx.from_arrow(pa.array(np.asarray(gids, dtype=np.uint32)))


def dev_batch(ctx, b, dtypes=F64):
    """the batch's arrays on the device, once for all accumulators that read them"""
    f = b["filter"]
    return (ctx.from_arrow(pa.array(b["a"], type=PA[dtypes[0]])), ctx.from_arrow(pa.array(b["b"], type=PA[dtypes[1]])), dev_ids(ctx, b["gids"]),
            None if f is None else ctx.from_arrow(pa.array(f, type=pa.bool_())), b["total"])


def check_values(kind, got, want, floor):
    """evaluate(): NULL exactly where the model is NULL, NaN exactly where it is NaN, an exact 0.0 of the model (CORR at count 1 or at a constant argument, SXX of a constant
    x ...) exactly 0.0, REGR_COUNT exact, else 1e-9 relative or within the floor"""
    assert len(got) == len(want), (kind, len(got), len(want))
    for g, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (kind, g, a, b)
        if b is None:
            continue
        if math.isnan(b) or math.isnan(a):
            assert math.isnan(a) and math.isnan(b), (kind, g, a, b)
        elif kind == "REGR_COUNT" or (kind == "CORR" and b == 0.0):
            assert a == b, (kind, g, a, b)
        else:
            assert cr.close(a, b, floor), (kind, g, a, b)


def check_state(acc, model, sa, sb):
    cols = [s.to_arrow() for s in acc.state()]
    names = cr.STATE_NAMES[model.family]
    assert len(cols) == len(names) and cols[0].type == pa.uint64() and all(c.type == pa.float64() for c in cols[1:]) and all(c.null_count == 0 for c in cols)
    want = model.state()
    assert cols[0].to_pylist() == want[0]
    for name, col, w, floor in zip(names[1:], cols[1:], want[1:], cr.state_floors(model.family, sa, sb)[1:]):
        for g, (a, b) in enumerate(zip(col.to_pylist(), w)):
            assert (math.isnan(a) and math.isnan(b)) or cr.close(a, b, floor), (name, g, a, b)


def check_against_model(ctx, kinds, batches, dtypes=F64, state=True):
    """every kind of `kinds` over the same batches: evaluate() and, per family once, the state columns"""
    dev = [dev_batch(ctx, b, dtypes) for b in batches]
    sa, sb = cr.scales(batches, dtypes)
    models, out = {}, {}
    for kind in kinds:
        acc = new_acc(ctx, kind, dtypes)
        for a, b, g, f, total in dev:
            acc.update_batch(a, b, g, f, total)
        fam = cr.family(kind)
        first = fam not in models
        if first:
            models[fam] = cr.model_of(kind, batches, dtypes)
        model = models[fam]
        assert len(model.accs) == batches[-1]["total"]
        check_values(kind, acc.evaluate().to_arrow().to_pylist(), model.evaluate(kind), cr.value_floor(kind, sa, sb))
        if first and state:
            check_state(acc, model, sa, sb)
            assert acc.size() >= 8 * len(cr.STATE_NAMES[fam]) * len(model.accs)
        out[kind] = acc
    return out, models


# ------------------------------------------------------------------ 1. the reference's known answers
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_answers(ctx, case):
    dtypes = tuple(case["dtypes"])
    if "a" in case:                                   # .slt: every output column of the query
        for kind, text in zip(case["kinds"], case["expected_text"]):
            acc = new_acc(ctx, kind, dtypes)
            acc.update_batch(*dev_batch(ctx, cr.batch(case["a"], case["b"], [0] * len(case["a"]), 1), dtypes))
            got = acc.evaluate().to_arrow().to_pylist()
            assert len(got) == 1 and ((got[0] is None) if text == "NULL" else (got[0] is not None and cr.close(got[0], float(text), 0.5e-12))), (case["ref"], kind, got)       # the file prints 12 decimals
        return
    accs = []
    for a, b in case["batches"]:
        if not accs or case["merge"]:
            accs.append(new_acc(ctx, case["kind"], dtypes))
        accs[-1].update_batch(*dev_batch(ctx, cr.batch(a, b, [0] * len(a), 1), dtypes))
    for other in accs[1:]:
        accs[0].merge_batch(other.state(), dev_ids(ctx, [0]), None, 1)
    got, want = accs[0].evaluate().to_arrow().to_pylist(), case["expected"]
    assert len(got) == 1 and ((got[0] is None) if want is None else (got[0] is not None and cr.close(got[0], want))), (case["ref"], got, want)


# ------------------------------------------------------------------ 2. both paths, every kind, ragged sizes
@pytest.mark.gpu
@pytest.mark.parametrize("total", cr.PATH_TOTALS)
def test_every_kind_on_both_paths(ctx, total):
    """all twelve kinds at 1, 2, S, S + 1, T and T + 1 groups over three ragged batches of a few thousand rows"""
    check_against_model(ctx, cr.KINDS, cr.ragged_batches(total))


@pytest.mark.gpu
@pytest.mark.parametrize("total", cr.PATH_TOTALS)
@pytest.mark.parametrize("n", cr.PATH_ROWS)
def test_paths_and_sizes(ctx, n, total):
    """0, 1, 63, 64, 65, 255, 256, 257 rows: a kind of each family, the others in turn"""
    turn = cr.PATH_ROWS.index(n) + cr.PATH_TOTALS.index(total)
    check_against_model(ctx, ("COVAR_POP", "CORR", cr.REGR_KINDS[turn % 9]), [cr.path_batch(n, total)])


@pytest.mark.gpu
@pytest.mark.parametrize("total", [9, S + 9, T + 1])
@pytest.mark.parametrize("ids", ["equal", "alternating"])
def test_wave_uniform_and_never_uniform_ids(ctx, ids, total):
    """all-equal ids: every wave takes the one-add-per-wave shortcut; strictly alternating ids: no wave does -- on the LDS and on the global path"""
    check_against_model(ctx, ("COVAR_SAMP", "CORR", "REGR_SLOPE", "REGR_INTERCEPT", "REGR_R2"), [cr.path_batch(4097, total, ids)])


# ------------------------------------------------------------------ 3. NULLs, filters, skipped ids, array views
@pytest.mark.gpu
def test_nulls_in_either_argument_filters_and_skipped_ids(ctx):
    b = cr.nulls_filters_batch()
    pairs = list(zip(b["a"], b["b"]))
    assert any(x is None and y is not None for x, y in pairs) and any(x is not None and y is None for x, y in pairs) and any(x is None and y is None for x, y in pairs)
    assert {True, False, None} <= set(b["filter"]) and cr.GID_NONE in b["gids"]
    accs, models = check_against_model(ctx, cr.KINDS, [b])
    assert models["REGR"].state()[0][0] == 0 and sum(models["REGR"].state()[0]) > 300         # group 0: no row with both arguments; the others count
    assert accs["REGR_COUNT"].evaluate().to_arrow().to_pylist()[0] == 0.0 and accs["CORR"].evaluate().to_arrow().to_pylist()[0] is None


@pytest.mark.gpu
def test_all_rows_null(ctx):
    n = 130
    for a, b in (([None] * n, [1.5] * n), ([1.5] * n, [None] * n), ([None] * n, [None] * n)):
        accs, _ = check_against_model(ctx, ONE_PER_FAMILY + ("REGR_COUNT",), [cr.batch(a, b, [i % 3 for i in range(n)], 3)])
        assert accs["REGR_COUNT"].evaluate().to_arrow().to_pylist() == [0.0, 0.0, 0.0] and accs["CORR"].evaluate().to_arrow().to_pylist() == [None, None, None]


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1, 64, 65])
def test_arguments_ids_and_filter_as_views(ctx, offset):
    """both arguments, the ids and the filter are windows `offset` rows into longer arrays (tests/views.py: the rows around the window hold NaN, infinities, extremes,
    valid bits and true Booleans); at offset 64 the windows with a bitmap are views that share their last word with the pad rows, at 1 and 65 they start inside a word"""
    from views import ViewCase
    b = cr.nulls_filters_batch(n=1300, total=29, seed=60 + offset, all_null_group=False)
    n = len(b["gids"])
    rng = np.random.default_rng(offset)
    nullable, plain = ViewCase(f"off{offset}", offset, n, "some"), ViewCase(f"ids-off{offset}", offset, n, "none")
    va, _ = nullable.make(ctx, None, rng, arr=pa.array(b["a"], type=pa.float64()))
    vb, _ = nullable.make(ctx, None, rng, arr=pa.array(b["b"], type=pa.float64()))
    vf, _ = nullable.make(ctx, None, rng, arr=pa.array(b["filter"], type=pa.bool_()))
    vg, _ = plain.make(ctx, None, rng, arr=pa.array(np.asarray(b["gids"], dtype=np.uint32)))
    sa, sb = cr.scales([b])
    for kind in ONE_PER_FAMILY:
        acc = new_acc(ctx, kind)
        acc.update_batch(va, vb, vg, vf, b["total"])
        model = cr.model_of(kind, [b])
        check_values(kind, acc.evaluate().to_arrow().to_pylist(), model.evaluate(), cr.value_floor(kind, sa, sb))
        check_state(acc, model, sa, sb)


# ------------------------------------------------------------------ 4. input types
@pytest.mark.gpu
@pytest.mark.parametrize("dtypes", cr.TYPE_PAIRS, ids=["x".join(p) for p in cr.TYPE_PAIRS])
def test_each_argument_is_cast_as_f64_on_its_own(ctx, dtypes):
    b = cr.typed_batch(dtypes)
    check_against_model(ctx, ONE_PER_FAMILY + ("REGR_SXX", "REGR_SYY", "REGR_AVGX"), [b], dtypes)
    import dfgpu
    acc = new_acc(ctx, "CORR", dtypes)
    a, bb, g, f, total = dev_batch(ctx, b, dtypes)
    if dtypes[0] != dtypes[1]:
        with pytest.raises(dfgpu.DfgpuError) as e:
            acc.update_batch(bb, a, g, f, total)                 # the arguments the other way round
        assert e.value.kind == "InvalidArgument"


@pytest.mark.gpu
def test_other_input_types_and_kinds_are_refused(ctx):
    import dfgpu
    capi = dfgpu.capi
    for ta, tb in ((capi.DECIMAL128, capi.FLOAT64), (capi.FLOAT64, capi.UTF8), (capi.BOOL, capi.BOOL), (capi.FLOAT64, capi.DATE32)):
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.CoMomentsAccumulator(ctx, capi.AGG_CORR, ta, tb)
        assert e.value.kind == "NotImplemented"
    for kind in (capi.AGG_SUM, capi.AGG_COUNT_DISTINCT, capi.AGG_STDDEV_POP, 10, 23):
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.CoMomentsAccumulator(ctx, kind, capi.FLOAT64, capi.FLOAT64)
        assert e.value.kind == "InvalidArgument"
    for kind in cr.KIND_CODES.values():                         # the one-argument accumulators do not know the new kinds
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.GroupsAccumulator(ctx, kind, capi.FLOAT64)
        assert e.value.kind == "InvalidArgument"
        with pytest.raises(dfgpu.DfgpuError) as e:
            dfgpu.MomentsAccumulator(ctx, kind, capi.FLOAT64)
        assert e.value.kind == "InvalidArgument"


# ------------------------------------------------------------------ 5. several batches, growing state
@pytest.mark.gpu
def test_three_batches_with_new_groups(ctx):
    batches = cr.growing_batches()
    assert batches[0]["total"] < batches[1]["total"] <= T < batches[2]["total"]
    accs, models = check_against_model(ctx, ONE_PER_FAMILY, batches)
    for kind in ONE_PER_FAMILY:
        acc = accs[kind]
        acc.update_batch(None, None, dev_ids(ctx, []), None, batches[2]["total"] + 5)          # a zero-row update grows the state
        st = [s.to_arrow().to_pylist() for s in acc.state()]
        assert st[0] == models[cr.family(kind)].state()[0] + [0] * 5 and all(col[-5:] == [0.0] * 5 for col in st[1:])
        assert acc.evaluate().to_arrow().to_pylist()[-5:] == [None] * 5


# ------------------------------------------------------------------ 6. a constant argument gives exact zeros
@pytest.mark.gpu
@pytest.mark.parametrize("total", [4, S + 1, T, T + 1])
def test_constant_argument_gives_exact_zeros(ctx, total):
    """0.1 in every row of a group -- group 0: argument 0 (y), group 1: argument 1 (x), group 2: both -- over three batches of more than 64 rows a group, next to groups that
    vary, on the LDS path with its small (4 groups) and its large arrays (S + 1, T groups) and on the global path (T + 1).  The reference keeps that argument's m2 and the group's algo_const at exactly 0.0 and branches on it:
    CORR is exactly 0.0, SLOPE / INTERCEPT / R2 are NULL where x is constant, SXX / SYY / SXY exactly 0.0.  A sum-then-divide batch mean of 0.1 is off in the last place,
    leaves an m2 of 1e-34 and turns these into huge numbers (tests/test_comoments_reference.py shows S / N != 0.1 for these counts)."""
    batches = cr.constant_batches(total)
    assert len(batches) == 3 and all(sum(1 for g in b["gids"] if g == k) > 64 for b in batches for k in (0, 1, 2))
    accs, models = check_against_model(ctx, cr.KINDS, batches)
    got = {k: a.evaluate().to_arrow().to_pylist() for k, a in accs.items()}
    assert got["CORR"][:3] == [0.0, 0.0, 0.0] and all(v is not None and v != 0.0 for v in got["CORR"][3:])
    for kind in ("REGR_SLOPE", "REGR_INTERCEPT", "REGR_R2"):
        assert got[kind][1] is None and got[kind][2] is None and all(v is not None for v in got[kind][3:]), kind
    assert got["REGR_SLOPE"][0] == 0.0 and got["REGR_R2"][0] is None and cr.close(got["REGR_INTERCEPT"][0], cr.CONSTANT)
    assert got["REGR_SXX"][1:3] == [0.0, 0.0] and got["REGR_SYY"][0] == 0.0 and got["REGR_SYY"][2] == 0.0 and got["REGR_SXY"][:3] == [0.0, 0.0, 0.0]
    assert got["COVAR_POP"][:3] == [0.0, 0.0, 0.0] and got["COVAR_SAMP"][:3] == [0.0, 0.0, 0.0]
    assert got["REGR_AVGY"][0] == cr.CONSTANT and got["REGR_AVGX"][1] == cr.CONSTANT and (got["REGR_AVGX"][2], got["REGR_AVGY"][2]) == (cr.CONSTANT, cr.CONSTANT)
    # and through a merge: the states of the three batches, taken one by one, merged in ONE call with three rows a group
    for kind in ("CORR", "REGR_SLOPE"):
        parts = []
        for b in batches:
            p = new_acc(ctx, kind); p.update_batch(*dev_batch(ctx, b)); parts.append([s.to_arrow() for s in p.state()])
        cols = [ctx.from_arrow(pa.concat_arrays([p[k] for p in parts])) for k in range(6)]
        merged = new_acc(ctx, kind)
        merged.merge_batch(cols, dev_ids(ctx, list(range(total)) * 3), None, total)
        v = merged.evaluate().to_arrow().to_pylist()
        assert (v[:3] == [0.0, 0.0, 0.0]) if kind == "CORR" else (v[0] == 0.0 and v[1] is None and v[2] is None), (kind, v[:3])


# ------------------------------------------------------------------ 7. merge
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["COVAR_POP", "CORR", "REGR_R2"])
def test_merge_device_and_model_states_into_a_third(ctx, kind):
    """every group appears three times in ONE merge_batch call (a Final stage sees a partial row per input partition): once from a state produced on the device, once from
    the model's state of the other input, once with count 0, which takes no part whatever its other columns say"""
    inputs = cr.merge_inputs()
    total = inputs[0]["total"]
    fam, ncols = cr.family(kind), len(cr.STATE_NAMES[cr.family(kind)])
    first = new_acc(ctx, kind); first.update_batch(*dev_batch(ctx, inputs[0]))
    dev_state = [s.to_arrow() for s in first.state()]
    pm = [cr.model_of(kind, [b]) for b in inputs]
    model_state = [pa.array(col, type=pa.uint64() if k == 0 else pa.float64()) for k, col in enumerate(pm[1].state())]
    empties = [pa.array([0, 0], type=pa.uint64())] + [pa.array([5.0, float("nan")]), pa.array([7.0, float("inf")])] * 3
    cols = [ctx.from_arrow(pa.concat_arrays([dev_state[k], empties[k], model_state[k]])) for k in range(ncols)]
    ids = list(range(total)) + [0, total - 1] + list(range(total))
    third = new_acc(ctx, kind)
    third.merge_batch(cols, dev_ids(ctx, ids), None, total)                        # into an empty accumulator
    model = cr.GroupedCoMoments(kind)
    model.merge_batch(pm[0].state(), list(range(total)), None, total)
    model.merge_batch(pm[1].state(), list(range(total)), None, total)
    sa, sb = cr.scales(inputs)
    floor = cr.value_floor(kind, sa, sb)
    check_values(kind, third.evaluate().to_arrow().to_pylist(), model.evaluate(), floor)
    check_state(third, model, sa, sb)
    check_values(kind, third.evaluate().to_arrow().to_pylist(), cr.model_of(kind, inputs).evaluate(), floor)          # and the merged answer is the answer over all rows
    # into an accumulator that holds rows already, with a filter and skipped ids
    rng = np.random.default_rng(9)
    filt = [[True, False, None][k] for k in rng.integers(0, 3, total)]
    gids = [cr.GID_NONE if r < 0.2 else g for g, r in zip(range(total), rng.random(total))]
    first.merge_batch([ctx.from_arrow(c) for c in model_state], dev_ids(ctx, gids), ctx.from_arrow(pa.array(filt, type=pa.bool_())), total)
    m4 = cr.model_of(kind, inputs[:1])
    m4.merge_batch(pm[1].state(), gids, filt, total)
    check_values(kind, first.evaluate().to_arrow().to_pylist(), m4.evaluate(), floor)
    check_state(first, m4, sa, sb)
    assert fam == m4.family


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["COVAR_SAMP", "CORR", "REGR_SXY"])
def test_malformed_states_are_refused_and_nothing_is_merged(ctx, kind):
    import dfgpu
    b = cr.path_batch(255, 9)
    acc = new_acc(ctx, kind); acc.update_batch(*dev_batch(ctx, b))
    before = [s.to_arrow() for s in acc.state()]
    ncols = len(before)
    assert ncols == (4 if kind == "COVAR_SAMP" else 6)
    good = [ctx.from_arrow(pa.array([2] * 9, type=pa.uint64()))] + [ctx.from_arrow(pa.array([1.0] * 9, type=pa.float64())) for _ in range(ncols - 1)]
    ids = dev_ids(ctx, list(range(9)))
    f32, u64, short = ctx.from_arrow(pa.array([1.0] * 9, type=pa.float32())), ctx.from_arrow(pa.array([3] * 9, type=pa.uint64())), ctx.from_arrow(pa.array([3.0] * 8, type=pa.float64()))
    bad = {"one column less": good[:-1], "one column more": good + good[1:2], "the other family's column count": (good + good[1:3]) if ncols == 4 else good[:4],
           "Int64 counts": [ctx.from_arrow(pa.array([2] * 9, type=pa.int64()))] + good[1:], "Float32 mean": [good[0], f32] + good[2:], "UInt64 last column": good[:-1] + [u64],
           "short last column": good[:-1] + [short], "short counts": [ctx.from_arrow(pa.array([2] * 8, type=pa.uint64()))] + good[1:]}
    for what, st in bad.items():
        with pytest.raises(dfgpu.DfgpuError) as e:
            acc.merge_batch(st, ids, None, 12)
        assert e.value.kind == "InvalidArgument", what
        after = [s.to_arrow() for s in acc.state()]
        assert all(x.equals(y) for x, y in zip(before, after)), what                 # not even grown to 12 groups
    acc.merge_batch(good, ids, None, 12)
    assert acc.state()[0].to_arrow().to_pylist() == [c + 2 for c in before[0].to_pylist()] + [0, 0, 0]


# ------------------------------------------------------------------ 8. an id beyond the groups
@pytest.mark.gpu
@pytest.mark.parametrize("total", [3, T + 5])
def test_group_id_out_of_range_is_the_accumulators_error(ctx, total):
    import dfgpu
    v = ctx.from_arrow(pa.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    g = dev_ids(ctx, [0, 1, total, 2, 1])
    for kind in ("COVAR_POP", "REGR_SLOPE"):
        with pytest.raises(dfgpu.DfgpuError) as e:
            new_acc(ctx, kind).update_batch(v, v, g, None, total)
        assert e.value.kind == "Execution" and "Arrow error: index out of bounds" in str(e.value)
        n = 4 if kind == "COVAR_POP" else 6
        st = [ctx.from_arrow(pa.array([1] * 5, type=pa.uint64()))] + [ctx.from_arrow(pa.array([1.0] * 5, type=pa.float64())) for _ in range(n - 1)]
        with pytest.raises(dfgpu.DfgpuError) as e:
            new_acc(ctx, kind).merge_batch(st, g, None, total)
        assert e.value.kind == "Execution" and "index out of bounds" in str(e.value)


# ------------------------------------------------------------------ 9. NaN and infinity
@pytest.mark.gpu
@pytest.mark.parametrize("total", [5, T + 1])
@pytest.mark.parametrize("side", ["a", "b"])
def test_nan_and_infinity_in_one_argument(ctx, side, total):
    """group 0 holds a NaN, group 1 +Inf and group 2 -Inf among finite values, group 3 only finite values, group 4 +Inf in EVERY row (a constant: the equal-extrema shortcut
    must not turn it into zeros): NaN exactly where the model's answer is NaN, NULL exactly where it is NULL"""
    inf, nan = float("inf"), float("nan")
    x = [1.0, nan, 2.0, 5.0, inf, 7.0, 1.5, -inf, 4.0, 1.5, 2.5, 4.0, inf, inf, inf]
    y = [3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0, 5.0, 3.0, 5.0, 8.0, 9.0, 7.0, 9.5]
    gids = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    b = cr.batch(x, y, gids, total) if side == "a" else cr.batch(y, x, gids, total)
    dev = dev_batch(ctx, b)
    sa, sb = cr.scales([b])
    models = {f: cr.model_of(k, [b]) for f, k in (("COVAR", "COVAR_POP"), ("CORR", "CORR"), ("REGR", "REGR_SXY"))}
    want = models["CORR"].evaluate()
    assert all(math.isnan(want[g]) for g in (0, 1, 2, 4)) and not math.isnan(want[3])
    own_m2, own_avg = ("REGR_SYY", "REGR_AVGY") if side == "a" else ("REGR_SXX", "REGR_AVGX")
    assert all(math.isnan(models["REGR"].evaluate(own_m2)[g]) for g in (0, 1, 2, 4))
    for kind in cr.KINDS:
        acc = new_acc(ctx, kind); acc.update_batch(*dev)
        got, want = acc.evaluate().to_arrow().to_pylist(), models[cr.family(kind)].evaluate(kind)
        if kind == own_avg:
            # the MEAN of an argument that holds an infinity is +-Inf or NaN in the reference, depending on where in the group the infinity stands (the recurrence
            # computes Inf - Inf once a later row follows); the device's mean is the sum's: not finite is all that can be asked of it
            for g in (1, 2, 4):
                assert got[g] is not None and not math.isfinite(got[g]), (kind, g, got[g])
                got[g] = want[g]
        check_values(kind, got, want, cr.value_floor(kind, sa, sb))


# ------------------------------------------------------------------ plan level
def table_of(t):
    return pa.table({"k": pa.array(t["k"], type=pa.int64()), "y": pa.array(t["y"], type=pa.float64()), "x": pa.array(t["x"], type=pa.float64()), "v": pa.array(t["v"], type=pa.int32()),
                     "f": pa.array(t["f"], type=pa.bool_()), "w": pa.array(t["w"], type=pa.float64())})


COL_TYPES = {"k": "INT64", "y": "FLOAT64", "x": "FLOAT64", "v": "INT32", "w": "FLOAT64"}


def agg_exprs(aggs, with_filters=True, names=("k", "y", "x", "v", "f", "w")):
    """aggs = [(fun, first column, second column or None, output name, filter column or None)]"""
    from dfgpu import capi, physical_plan as ops
    C, F = ops.Column, ops.Field
    out = []
    for fun, c1, c2, name, flt in aggs:
        two = {} if c2 is None else {"expr2": C(c2, names.index(c2)), "input_field2": F(c2, getattr(capi, COL_TYPES[c2]))}
        out.append(ops.AggregateFunctionExpr(fun, C(c1, names.index(c1)), name, filter=C(flt, names.index(flt)) if flt and with_filters else None,
                                             input_field=F(c1, getattr(capi, COL_TYPES[c1])), **two))
    return out


def agg_plan(ctx, partitions, keys, aggs, mode="Single", where=None):
    """partitions: lists of pyarrow tables.  Single: one AggregateExec over all partitions; PartialFinal: Partial per partition, then Final over them"""
    from dfgpu import physical_plan as ops
    names = partitions[0][0].column_names
    parts = [[ops.batch_from_arrow(ctx, t) for t in p] for p in partitions]
    src = ops.MemoryExec(parts, parts[0][0].schema)
    if where is not None:
        src = ops.FilterExec(where, src)
    C = ops.Column
    gb = [(C(k, names.index(k)), k) for k in keys]
    if mode == "Single":
        plan = ops.AggregateExec("Single", gb, agg_exprs(aggs), src)
    elif mode == "Partial":
        plan = ops.AggregateExec("Partial", gb, agg_exprs(aggs), src)
    else:
        plan = ops.AggregateExec("Final", [(C(k, i), k) for i, k in enumerate(keys)], agg_exprs(aggs, False), ops.AggregateExec("Partial", gb, agg_exprs(aggs), src))
    tc = ops.TaskContext(ctx, 8192)
    nparts = len(partitions) if mode == "Partial" else 1
    return pa.concat_tables([b.to_arrow() for p in range(nparts) for b in plan.execute(p, tc)])


TWO_ARG_AGGS = [(k, "y", "x", k.lower(), None) for k in cr.KINDS] + [("COVAR", "y", "x", "covar_f", "f"), ("CORR", "v", "x", "corr_vx", None), ("REGR_SLOPE", "y", "v", "slope_yv", "f")]
PLAIN_AGGS = [("SUM", "x", None, "sum", None), ("VAR_POP", "y", None, "var_pop", None), ("COUNT", "y", None, "count", None)]


def by_key(out, name):
    return dict(zip(out["k"].to_pylist(), out[name].to_pylist()))


def check_plan_output(out, plain, tables, keep=None):
    """every two-argument aggregate of TWO_ARG_AGGS against the model over the rows `keep` marks (None: all), group by group; SUM / VAR_POP / COUNT beside them equal
    what the plan without the new aggregates gives"""
    rows = [i for i in range(sum(len(t["k"]) for t in tables)) if keep is None or keep[i]]
    col = {c: [v for t in tables for v in t[c]] for c in ("k", "y", "x", "v", "f")}
    ids, table = cr.first_seen_ids([col["k"][i] for i in rows])
    total = len(table)
    assert sorted(out["k"].to_pylist(), key=repr) == sorted(table, key=repr) and out.num_rows == total == plain.num_rows
    for name in ("sum", "count"):
        assert by_key(out, name) == by_key(plain, name), name
    vp, vq = by_key(out, "var_pop"), by_key(plain, "var_pop")                  # Float64 atomics: the last bits vary from run to run
    assert all((vp[k] is None) == (vq[k] is None) and (vp[k] is None or cr.close(vp[k], vq[k])) for k in table)
    pick = lambda c: [col[c][i] for i in rows]
    inputs = {"yx": (cr.batch(pick("y"), pick("x"), ids, total), F64), "yx_f": (cr.batch(pick("y"), pick("x"), ids, total, pick("f")), F64),
              "vx": (cr.batch(pick("v"), pick("x"), ids, total), ("int32", "float64")), "yv_f": (cr.batch(pick("y"), pick("v"), ids, total, pick("f")), ("float64", "int32"))}
    which = {k.lower(): (k, "yx") for k in cr.KINDS}
    which.update(covar_f=("COVAR_SAMP", "yx_f"), corr_vx=("CORR", "vx"), slope_yv=("REGR_SLOPE", "yv_f"))
    models = {}
    for name, (kind, inp) in which.items():
        b, dtypes = inputs[inp]
        key = (cr.family(kind), inp)
        if key not in models:
            models[key] = cr.model_of(kind, [b], dtypes)
        sa, sb = cr.scales([b], dtypes)
        got = by_key(out, name)
        assert out.schema.field(name).type == pa.float64()
        check_values(kind, [got[k] for k in table], models[key].evaluate(kind), cr.value_floor(kind, sa, sb))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Single", "PartialFinal"])
def test_plan_grouped(ctx, mode):
    """3 batches of 4000 rows in 2 partitions, 40 groups and the NULL key group: the twelve kinds over (y, x), COVAR under FILTER (WHERE f), CORR over an Int32 and a
    Float64 column, REGR_SLOPE over a Float64 and an Int32 column under a filter, with SUM, VAR_POP and COUNT beside them in ONE AggregateExec.  Single and
    Partial -> Final over the two partitions give the same answers (each against the model over all rows); x and y hold multiples of 1/64, so SUM(x) is exact in any order
    and must EQUAL what the plan without the new aggregates gives."""
    tables = cr.plan_tables()
    pt = [table_of(t) for t in tables]
    parts = [[pt[0], pt[1]], [pt[2]]]
    out = agg_plan(ctx, parts, ["k"], TWO_ARG_AGGS + PLAIN_AGGS, mode)
    plain = agg_plan(ctx, parts, ["k"], PLAIN_AGGS, mode)
    assert out.column_names == ["k"] + [a[3] for a in TWO_ARG_AGGS + PLAIN_AGGS] and out.num_rows == 41 and None in out["k"].to_pylist()
    check_plan_output(out, plain, tables)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Single", "PartialFinal"])
def test_plan_above_a_fused_filter(ctx, mode):
    """FilterExec(w > -5) directly above the scan: its selection reaches the aggregate as a row mask, not as compacted batches -- grouped and without GROUP BY"""
    from dfgpu import physical_plan as ops
    tables = cr.plan_tables(seed=8, batches=2, rows=1500, groups=12)
    pt = [table_of(t) for t in tables]
    where = ops.BinaryExpr(ops.Column("w", 5), ">", ops.Literal(-5.0, pa.float64()))
    keep = [w > -5.0 for t in tables for w in t["w"]]
    assert 0.5 < sum(keep) / len(keep) < 0.95
    out = agg_plan(ctx, [[pt[0]], [pt[1]]], ["k"], TWO_ARG_AGGS + PLAIN_AGGS, mode, where)
    plain = agg_plan(ctx, [[pt[0]], [pt[1]]], ["k"], PLAIN_AGGS, mode, where)
    check_plan_output(out, plain, tables, keep)
    # no GROUP BY: one group, the rows the FilterExec drops must not reach it
    aggs = [("CORR", "y", "x", "corr", None), ("REGR_COUNT", "y", "x", "n", "f"), ("COVAR_POP", "y", "x", "covar_pop", None)]
    out = agg_plan(ctx, [[pt[0]], [pt[1]]], [], aggs, mode, where)
    rows = [i for i, kp in enumerate(keep) if kp]
    y, x, f = ([v for t in tables for v in t[c]] for c in ("y", "x", "f"))
    b = cr.batch([y[i] for i in rows], [x[i] for i in rows], [0] * len(rows), 1)
    bf = dict(b, filter=[f[i] for i in rows])
    sa, sb = cr.scales([b])
    assert out.num_rows == 1
    check_values("CORR", out["corr"].to_pylist(), cr.model_of("CORR", [b]).evaluate(), 1e-9)
    check_values("COVAR_POP", out["covar_pop"].to_pylist(), cr.model_of("COVAR_POP", [b]).evaluate(), cr.value_floor("COVAR_POP", sa, sb))
    assert out["n"].to_pylist() == cr.model_of("REGR_COUNT", [bf]).evaluate() and 0 < out["n"][0].as_py() < len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Single", "PartialFinal"])
def test_plan_without_group_by(ctx, mode):
    empty = table_of({c: [] for c in ("k", "y", "x", "v", "f", "w")})
    aggs = [(k, "y", "x", k.lower(), None) for k in cr.KINDS]
    out = agg_plan(ctx, [[empty]], [], aggs, mode)
    assert out.num_rows == 1 and [out[k.lower()][0].as_py() for k in cr.KINDS] == [0.0 if k == "REGR_COUNT" else None for k in cr.KINDS]
    one = table_of({"k": [1], "y": [3.5], "x": [1.25], "v": [1], "f": [True], "w": [0.0]})
    out = agg_plan(ctx, [[one]], [], aggs, mode)
    want = {"COVAR_SAMP": None, "COVAR_POP": 0.0, "CORR": 0.0, "REGR_SLOPE": None, "REGR_INTERCEPT": None, "REGR_COUNT": 1.0, "REGR_R2": None, "REGR_AVGX": 1.25, "REGR_AVGY": 3.5,
            "REGR_SXX": 0.0, "REGR_SYY": 0.0, "REGR_SXY": 0.0}
    assert out.num_rows == 1 and {k: out[k.lower()][0].as_py() for k in cr.KINDS} == want
    tables = cr.plan_tables(seed=6, batches=2, rows=700)
    out = agg_plan(ctx, [[table_of(tables[0])], [table_of(tables[1])]], [], aggs, mode)
    y, x = [v for t in tables for v in t["y"]], [v for t in tables for v in t["x"]]
    b = cr.batch(y, x, [0] * len(y), 1)
    sa, sb = cr.scales([b])
    models = {f: cr.model_of(k, [b]) for f, k in (("COVAR", "COVAR_POP"), ("CORR", "CORR"), ("REGR", "REGR_SXY"))}
    for kind in cr.KINDS:
        check_values(kind, out[kind.lower()].to_pylist(), models[cr.family(kind)].evaluate(kind), cr.value_floor(kind, sa, sb))


@pytest.mark.gpu
def test_partial_stage_schema(ctx):
    """the Partial stage emits the reference's state columns per kind, by name, order and type, without NULLs, also for a group without a pair (covariance.rs:86-108,
    correlation.rs:77-108, regr.rs:131-162); REGR lists x, its SECOND argument, first"""
    t = table_of({"k": [1, 1, 2, 3, 3, 3], "y": [1.0, 2.0, None, 4.0, 6.0, 8.0], "x": [10.0, 30.0, 5.0, 1.0, None, 3.0], "v": [0] * 6, "f": [True] * 6, "w": [0.0] * 6})
    aggs = [("COVAR_POP", "y", "x", "c", None), ("SUM", "x", None, "s", None), ("CORR", "y", "x", "r", None), ("REGR_AVGX", "y", "x", "g", None)]
    out = agg_plan(ctx, [[t]], ["k"], aggs, "Partial")
    names = ["k"] + [f"c[{n}]" for n in cr.STATE_NAMES["COVAR"]] + ["s[sum]"] + [f"r[{n}]" for n in cr.STATE_NAMES["CORR"]] + [f"g[{n}]" for n in cr.STATE_NAMES["REGR"]]
    assert out.column_names == names
    for name in names[1:]:
        if name != "s[sum]":
            assert out.schema.field(name).type == (pa.uint64() if name.endswith("[count]") else pa.float64()) and out[name].null_count == 0, name
    assert out["c[count]"].to_pylist() == out["r[count]"].to_pylist() == out["g[count]"].to_pylist() == [2, 0, 2]
    want = {"c[mean1]": [1.5, 0.0, 6.0], "c[mean2]": [20.0, 0.0, 2.0], "c[algo_const]": [10.0, 0.0, 4.0], "r[mean1]": [1.5, 0.0, 6.0], "r[m2_1]": [0.5, 0.0, 8.0], "r[mean2]": [20.0, 0.0, 2.0],
            "r[m2_2]": [200.0, 0.0, 2.0], "r[algo_const]": [10.0, 0.0, 4.0], "g[mean_x]": [20.0, 0.0, 2.0], "g[mean_y]": [1.5, 0.0, 6.0], "g[m2_x]": [200.0, 0.0, 2.0],
            "g[m2_y]": [0.5, 0.0, 8.0], "g[algo_const]": [10.0, 0.0, 4.0]}
    for name, w in want.items():
        assert all(cr.close(a, b) for a, b in zip(out[name].to_pylist(), w)), (name, out[name].to_pylist())


@pytest.mark.gpu
def test_grouping_sets_missing_and_surplus_second_arguments_are_refused(ctx):
    import dfgpu
    from dfgpu import capi, physical_plan as ops
    t = table_of(cr.plan_tables(seed=7, batches=1, rows=50)[0])
    b = ops.batch_from_arrow(ctx, t)
    C, F, L = ops.Column, ops.Field, ops.Literal
    tc = ops.TaskContext(ctx, 8192)
    src = lambda: ops.MemoryExec([[b]], b.schema)
    two = lambda fun, name, **kw: ops.AggregateFunctionExpr(fun, C("y", 1), name, input_field=F("y", capi.FLOAT64), **kw)
    x2 = {"expr2": C("x", 2), "input_field2": F("x", capi.FLOAT64)}
    gb = ops.PhysicalGroupBy([(C("k", 0), "k")], [(L(None, pa.int64()), "k")], [[False], [True]])
    for fun in ("CORR", "COVAR_POP", "REGR_SXY"):
        with pytest.raises(dfgpu.DfgpuError) as e:
            list(ops.AggregateExec("Single", gb, [two(fun, "rho", **x2)], src()).execute(0, tc))
        assert e.value.kind == "NotImplemented" and "grouping sets" in str(e.value) and "rho" in str(e.value)
    # a two-argument kind without its second argument: refused when the plan executes, by name
    for mode in ("Single", "Partial"):
        with pytest.raises(dfgpu.DfgpuError) as e:
            list(ops.AggregateExec(mode, [(C("k", 0), "k")], [two("REGR_SLOPE", "lonely")], src()).execute(0, tc))
        assert e.value.kind == "InvalidArgument" and "lonely" in str(e.value)
    # a second argument on a one-argument kind
    with pytest.raises(dfgpu.DfgpuError) as e:
        list(ops.AggregateExec("Single", [(C("k", 0), "k")], [two("VAR_POP", "crowded", **x2)], src()).execute(0, tc))
    assert e.value.kind == "InvalidArgument" and "crowded" in str(e.value)
    # argument types: the first when the aggregate is built, the second when it is attached
    for typ in (capi.UTF8, capi.DECIMAL128, capi.BOOL, capi.DATE32):
        for bad_first in (True, False):
            f1, f2 = (F("y", typ, 10, 2), F("x", capi.FLOAT64)) if bad_first else (F("y", capi.FLOAT64), F("x", typ, 10, 2))
            agg = ops.AggregateFunctionExpr("CORR", C("y", 1), "a", input_field=f1, expr2=C("x", 2), input_field2=f2)
            with pytest.raises(dfgpu.DfgpuError) as e:
                list(ops.AggregateExec("Final", [(C("k", 0), "k")], [agg], src()).execute(0, tc))
            assert e.value.kind == "NotImplemented" and f"kind {capi.AGG_CORR}" in str(e.value) and f"type {typ}" in str(e.value)
    # and with everything in place the same plan runs, also as a fresh copy of itself
    plan = ops.AggregateExec("Single", [(C("k", 0), "k")], [two("CORR", "rho", **x2)], src())
    first = pa.concat_tables([o.to_arrow() for o in plan.execute(0, tc)])
    again = pa.concat_tables([o.to_arrow() for o in ops.with_fresh_state(plan).execute(0, tc)])          # the copy carries the second argument
    assert first.num_rows > 1 and first.column_names == again.column_names == ["k", "rho"] and first["k"].to_pylist() == again["k"].to_pylist()
    assert all((a is None) == (b is None) and (a is None or abs(a - b) <= 1e-9) for a, b in zip(first["rho"].to_pylist(), again["rho"].to_pylist()))
