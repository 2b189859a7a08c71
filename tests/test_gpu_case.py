"""-m gpu: CASE WHEN on the device -- dfgpu_case (k_case_select / k_case_index), the row-selection stack and CaseExpr through plans.
Expected answers come from case_rows (tests/case_reference.py, pinned by tests/test_case_reference.py); every comparison is bit-exact."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

from case_reference import PA_TYPES, batch_column, case_rows, load_vectors, vector_case_rows
from test_gpu_core import plain, rand_array
from test_gpu_expr import OPCODE, exported, same
from views import CLASS_A, CLASS_C, CLASS_C_EDGE, CLASS_E, ViewCase

pytestmark = pytest.mark.gpu
KINDS = ["int8", "int16", "int32", "int64", "uint64", "float32", "float64", "date32", "decimal", "bool", "utf8", "dict"]
# k_case_select gives one wave case_rows<T>() = 8 consecutive 64-row groups (4 for 16-byte elements), so a wave's chunk is 512 rows (256 for Decimal128) and a
# workgroup of 4 waves covers 2048 (1024): a chunk less one row, exactly, and one more; 2597 = a full workgroup, a full chunk and a ragged tail
LENGTHS = [0, 1, 63, 64, 65, 127, 4097, 255, 256, 257, 511, 512, 513, 2597]


class Operands:
    """One CASE over host arrays.  conds[k]: Boolean arrays of n rows; thens[k] / else_: (array, is_scalar) or None (the untyped NULL literal / no ELSE).
    Dictionary operands have to share one dictionary, so they are windows of one imported parent."""

    def __init__(self, kind, n, nb, else_mode, rng, then_modes=None, null_frac=0.2, cond_null_frac=0.15):
        self.kind, self.n = kind, n
        self.conds = [pa.array(rng.random(n) < 0.3, mask=(rng.random(n) < cond_null_frac) if cond_null_frac else None) for _ in range(nb)]
        modes = then_modes if then_modes is not None else [["column", "scalar", "column", "null"][(k + nb) % 4] if nb > 1 else "column" for k in range(nb)]
        if all(m == "null" for m in modes) and else_mode == "none":
            modes[0] = "column"
        self.modes, self.else_mode = modes, else_mode
        lens = [n if m == "column" else 1 if m == "scalar" else 0 for m in modes + [else_mode]]
        self.stride = ((max(n, 1) + 63) // 64) * 64                      # every window starts on a bitmap word of its own
        pool = rand_array(kind, self.stride * len(lens), null_frac, rng)
        self.pool, self.lens = pool, lens
        self.ops = [pool.slice(j * self.stride, l) if m in ("column", "scalar") else None for j, (m, l) in enumerate(zip(modes + [else_mode], lens))]

    def expected(self):
        rows = lambda a, m: None if a is None else (plain(a).to_pylist() * self.n if m == "scalar" else plain(a).to_pylist())
        thens = [rows(a, m) for a, m in zip(self.ops[:-1], self.modes)]
        out = case_rows([c.to_pylist() for c in self.conds], thens, rows(self.ops[-1], self.else_mode)) if self.n else []
        return pa.array(out, type=plain(self.pool).type)

    def device(self, ctx):
        if self.kind == "dict":
            parent = ctx.from_arrow(self.pool)
            arrs = [parent.slice(j * self.stride, l) if a is not None else None for j, (a, l) in enumerate(zip(self.ops, self.lens))]
        else:
            arrs = [ctx.from_arrow(a) if a is not None else None for a in self.ops]
        out = ctx.case([ctx.from_arrow(c) for c in self.conds], arrs[:-1], arrs[-1], [m == "scalar" for m in self.modes], self.else_mode == "scalar")
        return exported(ctx, out)


def check(ctx, o):
    got, want = o.device(ctx), o.expected()
    if o.kind == "dict":
        assert pa.types.is_dictionary(got.type)
        got = plain(got)
    assert len(got) == o.n and same(got, want), f"{o.kind} n={o.n} thens={o.modes} else={o.else_mode}"


@pytest.mark.parametrize("else_mode", ["none", "column", "scalar"])
@pytest.mark.parametrize("nb", [1, 2, 8, 9, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_case_random(ctx, kind, nb, else_mode):
    """1 .. 17 branches: one launch, one launch that is full, and one and two continuations whose result is the ELSE of the launch in front"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 10 * nb + len(else_mode))
    check(ctx, Operands(kind, 1000, nb, else_mode, rng))


@pytest.mark.parametrize("kind", ["int32", "float64", "decimal", "bool", "utf8", "dict"])
@pytest.mark.parametrize("modes", [(a, b) for a in ("column", "scalar", "null") for b in ("column", "scalar", "null")])
def test_case_every_operand_mix(ctx, kind, modes):
    rng = np.random.default_rng(5)
    for else_mode in ("none", "column", "scalar"):
        check(ctx, Operands(kind, 777, 2, else_mode, rng, then_modes=list(modes)))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["int8", "int64", "decimal", "bool", "utf8"])
def test_case_lengths(ctx, kind, n):
    rng = np.random.default_rng(n + 1)
    check(ctx, Operands(kind, n, 3, "column", rng, then_modes=["column", "scalar", "column"]))
    check(ctx, Operands(kind, n, 1, "none", rng))


@pytest.mark.parametrize("pattern", ["all_false", "all_true", "one_group", "all_null"])
@pytest.mark.parametrize("kind", ["int64", "decimal", "bool", "utf8"])
def test_case_uniform_when_words_and_poison(ctx, kind, pattern):
    """WHEN words that are the same for a whole 64-row group, and operand columns whose rows OUTSIDE their branch hold valid extreme values: none may show"""
    n = 1000
    rng = np.random.default_rng(3)
    bits = {"all_false": np.zeros(n, bool), "all_true": np.ones(n, bool), "one_group": (np.arange(n) // 64) == 7, "all_null": np.ones(n, bool)}[pattern]
    cond = pa.array(bits, mask=np.ones(n, bool) if pattern == "all_null" else None)
    taken = bits & (pattern != "all_null")
    good = rand_array(kind, 2 * n, 0.0, rng)
    poison = {"int64": 2**63 - 1, "decimal": decimal.Decimal(10**15 - 1).scaleb(-2), "bool": None, "utf8": "POISON"}[kind]
    if kind == "bool":                       # a Boolean has no spare value: the branch's own rows are all False, the others True
        then = pa.array(~taken)
        els = pa.array(taken)
        want = pa.array(np.zeros(n, bool))
    else:
        g = good.to_pylist()
        then = pa.array([g[i] if taken[i] else poison for i in range(n)], type=good.type)
        els = pa.array([poison if taken[i] else g[n + i] for i in range(n)], type=good.type)
        want = pa.array([g[i] if taken[i] else g[n + i] for i in range(n)], type=good.type)
    got = exported(ctx, ctx.case([ctx.from_arrow(cond)], [ctx.from_arrow(then)], ctx.from_arrow(els)))
    assert same(got, want)
    assert got.to_pylist() == case_rows([cond.to_pylist()], [then.to_pylist()], els.to_pylist())
    if kind != "bool":
        assert poison not in got.to_pylist()


VIEW_CASES = [CLASS_A[0], CLASS_A[3], CLASS_C[1], CLASS_C[5], CLASS_C_EDGE[0], CLASS_C_EDGE[1], CLASS_E[0]]


@pytest.mark.parametrize("vc", VIEW_CASES, ids=[v.id for v in VIEW_CASES])
@pytest.mark.parametrize("kind", ["int8", "int64", "decimal", "bool", "utf8"])
def test_case_on_views(ctx, kind, vc):
    """THEN / ELSE windows at odd rows (values aligned to the element only), WHEN bitmaps and nullable operands whose last word continues with the parent's live
    bits (class C), the copying slice as control (class E).  A Boolean result then serves as a mask (exported), so stray tail bits show."""
    rng = np.random.default_rng(17)
    wc = ViewCase(vc.id + "-when", vc.off, vc.n, "some" if vc.nulls == "none" else vc.nulls)
    conds = [wc.make(ctx, "bool", rng) for _ in range(2)]
    vals = [vc.make(ctx, kind, rng) for _ in range(3)]
    out = ctx.case([c[0] for c in conds], [vals[0][0], vals[1][0]], vals[2][0])
    got = exported(ctx, out)
    want = case_rows([c[1].to_pylist() for c in conds], [plain(vals[0][1]).to_pylist(), plain(vals[1][1]).to_pylist()], plain(vals[2][1]).to_pylist())
    assert same(plain(got), pa.array(want, type=plain(vals[0][1]).type))
    # no ELSE: the validity also comes from the masks
    got = exported(ctx, ctx.case([conds[0][0]], [vals[0][0]]))
    assert same(plain(got), pa.array(case_rows([conds[0][1].to_pylist()], [plain(vals[0][1]).to_pylist()]), type=plain(vals[0][1]).type))


def test_case_decimal_in_memory_aligned_to_8_bytes(ctx):
    """Decimal128 operands that start 8 bytes off a 16-byte boundary (memory wrapped from outside only has to be 8-byte aligned): the two-load variant of the
    16-byte kernel runs, and gives what the aligned one gives"""
    import torch
    from dfgpu import capi
    n = 1000
    rng = np.random.default_rng(23)
    cond = pa.array(rng.random(n) < 0.5)
    a, b = rand_array("decimal", n, 0.0, rng), rand_array("decimal", n, 0.0, rng)

    def off_by_8(arr):
        words = torch.from_numpy(np.concatenate([[0], np.frombuffer(arr.buffers()[1], dtype=np.int64, count=2 * n)]).astype(np.int64)).cuda()
        assert words[1:].data_ptr() % 16 == 8
        return ctx.wrap_tensor(words[1:], capi.DECIMAL128, 15, 2)
    want = pa.array(case_rows([cond.to_pylist()], [a.to_pylist()], b.to_pylist()), type=a.type)
    got = ctx.case([ctx.from_arrow(cond)], [off_by_8(a)], off_by_8(b)).to_arrow()
    assert same(got, want)
    assert same(ctx.case([ctx.from_arrow(cond)], [ctx.from_arrow(a)], ctx.from_arrow(b)).to_arrow(), want)


def test_case_else_is_cast_to_the_type_of_the_thens(ctx):
    cond = pa.array([True, False, None, False])
    then = pa.array([1.5, 2.5, 3.5, 4.5])
    got = ctx.case([ctx.from_arrow(cond)], [ctx.from_arrow(then)], ctx.from_arrow(pa.array([999], type=pa.int32())), else_scalar=True).to_arrow()
    assert same(got, pa.array([1.5, 999.0, 999.0, 999.0]))
    got = ctx.case([ctx.from_arrow(cond)], [None], ctx.from_arrow(pa.array([7, 8, 9, 10], type=pa.int32()))).to_arrow()       # the type comes from the ELSE
    assert same(got, pa.array([None, 8, 9, 10], type=pa.int32()))


def test_case_argument_errors(ctx):
    import dfgpu
    f = ctx.from_arrow
    cond, i64, f64 = f(pa.array([True, False, True])), f(pa.array([1, 2, 3])), f(pa.array([1.0, 2.0, 3.0]))
    d2 = f(pa.array([decimal.Decimal("1.00")] * 3, type=pa.decimal128(15, 2)))
    d3 = f(pa.array([decimal.Decimal("1.000")] * 3, type=pa.decimal128(15, 3)))
    cases = [(lambda: ctx.case([cond, cond], [i64, f64]), "THEN 1 has type 11, expected 5"),
             (lambda: ctx.case([cond, cond], [d2, d3]), r"THEN 1 is Decimal128\(15, 3\), expected Decimal128\(15, 2\)"),
             (lambda: ctx.case([cond, f(pa.array([True, False]))], [i64, i64]), "WHEN 1 has 2 rows, expected 3"),
             (lambda: ctx.case([i64], [i64]), "WHEN 0 is not a Boolean array"),
             (lambda: ctx.case([], []), "There must be at least one WHEN clause"),
             (lambda: ctx.case([cond], [None]), "untyped NULL literal"),
             (lambda: ctx.case([cond], [f(pa.array([1, 2]))]), "THEN 0 has 2 rows, expected 3")]
    for call, message in cases:
        with pytest.raises(dfgpu.DfgpuError, match=message) as e:
            call()
        assert e.value.status == 5
    other = pa.array(["a", "b", "c"]).dictionary_encode()
    with pytest.raises(dfgpu.DfgpuError) as e:             # dictionaries that do not share their parent: what dfgpu_concat declines
        ctx.case([cond], [f(other)], f(pa.array(["x", "y", "z"]).dictionary_encode()))
    assert e.value.status == 4


# ------------------------------------------------------------------ the row-selection stack
def divides(ctx, a, b):
    return ctx.binary(OPCODE["/"], a, b).to_arrow()


def test_row_selection_stack(ctx):
    import dfgpu
    f = ctx.from_arrow
    n = 200
    a = f(pa.array(np.full(n, 100, dtype=np.int32)))
    bv = np.ones(n, dtype=np.int32); bv[[5, 70, 130]] = 0
    b = f(pa.array(bv))
    sel = lambda *drop: f(pa.array(~np.isin(np.arange(n), drop)))

    def set_selection(mask):                                 # `mask` stays referenced until the call is over
        ctx.check(ctx.lib.dfgpu_ctx_set_row_selection(ctx.h, mask.h if mask is not None else None))

    def raises():
        try:
            divides(ctx, a, b)
            return False
        except dfgpu.DfgpuError as e:
            assert "Divide by zero" in str(e)
            return True
    try:
        assert raises()
        with pytest.raises(dfgpu.DfgpuError) as e:
            ctx.pop_row_selection()                          # nothing pushed
        assert e.value.status == 5
        with pytest.raises(dfgpu.DfgpuError) as e:
            ctx.push_row_selection(None)
        assert e.value.status == 5
        ctx.push_row_selection(sel(5, 70))                   # no selection set: the mask itself
        assert raises()
        ctx.push_row_selection(sel(130))                     # nested: the intersection
        assert not raises()
        ctx.pop_row_selection()
        assert raises()                                      # row 130 is selected again
        ctx.pop_row_selection()
        set_selection(sel(5, 130))
        with pytest.raises(dfgpu.DfgpuError) as e:
            ctx.push_row_selection(f(pa.array([True, False])))      # another length than the selection's
        assert e.value.status == 5
        ctx.push_row_selection(sel(70))
        assert not raises()
        ctx.pop_row_selection()
        assert raises()                                      # exactly where it raised before the balanced push / pop: row 70
        ctx.push_row_selection(sel(70))
        set_selection(sel(5, 70, 130))       # set replaces the bottom and drops what was pushed
        with pytest.raises(dfgpu.DfgpuError):
            ctx.pop_row_selection()
        assert not raises()
        ctx.push_row_selection(sel(1))
        set_selection(None)                                  # NULL clears everything
        with pytest.raises(dfgpu.DfgpuError):
            ctx.pop_row_selection()
        assert raises()
    finally:
        set_selection(None)


# ------------------------------------------------------------------ CaseExpr through plans
def build_expr(ops, e, index):
    if e is None:
        return None
    if e[0] == "col":
        return ops.Column(e[1], index[e[1]])
    if e[0] == "lit":
        return ops.Literal(e[2], PA_TYPES[e[1]])
    if e[0] == "cast":
        from dfgpu import capi
        return ops.CastExpr(build_expr(ops, e[1], index), {"float64": capi.FLOAT64, "int32": capi.INT32}[e[2]])
    return ops.BinaryExpr(build_expr(ops, e[1], index), e[0], build_expr(ops, e[2], index))


def project(ctx, task_ctx, table, exprs, predicate=None):
    from dfgpu import physical_plan as ops
    batch = ops.batch_from_arrow(ctx, table)
    src = ops.MemoryExec([[batch]], batch.schema)
    if predicate is not None:
        src = ops.FilterExec(predicate, src)
    out = ops.collect(ops.ProjectionExec([(e, f"c{i}") for i, e in enumerate(exprs)], src), task_ctx)
    return [pa.concat_arrays([b.columns[i].to_arrow() for b in out]) for i in range(len(exprs))]


VECTORS = load_vectors()


@pytest.mark.parametrize("vec", VECTORS, ids=[v["name"] for v in VECTORS])
def test_case_expr_reference_vectors(ctx, task_ctx, vec):
    from dfgpu import physical_plan as ops
    col = batch_column(vec)
    index = {vec["batch"]["column"]: 0}
    e = ops.CaseExpr(build_expr(ops, vec["base"], index), [(build_expr(ops, w, index), build_expr(ops, t, index)) for w, t in vec["when_then"]], build_expr(ops, vec["else"], index))
    got, = project(ctx, task_ctx, pa.table({vec["batch"]["column"]: col}), [e])
    want = pa.array(vec["expected"], type=PA_TYPES[vec["type"]])
    assert same(got, want)
    rows, typ = vector_case_rows(vec)
    assert same(got, pa.array(rows, type=typ))


def i32(v):
    return pa.array(np.asarray(v, dtype=np.int32))


def test_case_expr_short_circuit(ctx, task_ctx):
    """Int32: `/` is checked.  A branch may raise only on the rows that reach it."""
    import dfgpu
    from dfgpu import physical_plan as ops
    C, B, L = ops.Column, ops.BinaryExpr, lambda v: ops.Literal(v, pa.int32())
    rng = np.random.default_rng(29)
    a = rng.integers(-12, 13, 3000).astype(np.int32)
    assert (a == 0).any()
    t = pa.table({"a": i32(a)})
    div = B(L(100), "/", C("a", 0))
    with pytest.raises(dfgpu.DfgpuError, match="Divide by zero"):
        project(ctx, task_ctx, t, [div])
    quot = np.fix(100.0 / np.where(a == 0, 1, a)).astype(np.int32)
    got, = project(ctx, task_ctx, t, [ops.CaseExpr(None, [(B(C("a", 0), "!=", L(0)), div)], L(-1))])
    assert same(got, i32(np.where(a != 0, quot, -1)))
    # the unsafe WHEN runs under the remainder: rows with a = 0 were taken by the branch in front
    got, = project(ctx, task_ctx, t, [ops.CaseExpr(None, [(B(C("a", 0), "=", L(0)), L(0)), (B(div, ">", L(3)), L(1))], None)])
    want = case_rows([(a == 0).tolist(), (quot > 3).tolist()], [[0] * len(a), [1] * len(a)])
    assert same(got, pa.array(want, type=pa.int32()))
    # with a base expression, and a NULL base that goes to the ELSE without reaching the WHENs
    an = pa.array(a, mask=(np.arange(len(a)) % 11 == 0))
    got, = project(ctx, task_ctx, pa.table({"a": an}), [ops.CaseExpr(C("a", 0), [(L(0), L(-7)), (B(L(100), "/", C("a", 0)), L(10))], L(5))])
    rows = [5 if v is None else -7 if v == 0 else 10 if int(100 / v) == v else 5 for v in an.to_pylist()]
    assert same(got, pa.array(rows, type=pa.int32()))
    # a row that reaches the division with a zero still fails
    with pytest.raises(dfgpu.DfgpuError, match="Divide by zero"):
        project(ctx, task_ctx, t, [ops.CaseExpr(None, [(B(C("a", 0), ">", L(5)), L(1))], div)])
    with pytest.raises(dfgpu.DfgpuError, match="Divide by zero"):
        project(ctx, task_ctx, t, [ops.CaseExpr(None, [(B(C("a", 0), "<", L(5)), div)], L(1))])
    # and the row selection is as it was: the bare division raises again, nothing is left pushed
    with pytest.raises(dfgpu.DfgpuError, match="Divide by zero"):
        project(ctx, task_ctx, t, [div])
    with pytest.raises(dfgpu.DfgpuError):
        ctx.pop_row_selection()


def test_case_expr_under_a_carried_selection(ctx, task_ctx):
    """FilterExec keeps 3/4 of the rows, so ProjectionExec carries the selection instead of compacting.  A dropped row has b = 1, a = 0 under
    WHEN b = 1 THEN 100 / a: the pushed mask intersects the selection, so it cannot raise.  A later expression of the same projection runs under the
    restored selection: a dropped zero does not raise there, a kept one does."""
    import dfgpu
    from dfgpu import physical_plan as ops
    C, B, L = ops.Column, ops.BinaryExpr, lambda v: ops.Literal(v, pa.int32())
    n = 4000
    rng = np.random.default_rng(31)
    keep = rng.random(n) < 0.75
    a = rng.integers(1, 50, n).astype(np.int32) * rng.choice([-1, 1], n).astype(np.int32)
    b = rng.integers(0, 3, n).astype(np.int32)
    a2 = rng.integers(1, 50, n).astype(np.int32)
    a[~keep] = 0; b[~keep] = 1; a2[~keep] = 0
    case = ops.CaseExpr(None, [(B(C("b", 1), "=", L(1)), B(L(100), "/", C("a", 0)))], L(-1))
    exprs = [case, B(L(100), "/", C("a2", 2))]
    t = pa.table({"a": i32(a), "b": i32(b), "a2": i32(a2), "keep": pa.array(keep)})
    got = project(ctx, task_ctx, t, exprs, predicate=C("keep", 3))
    ka, kb, ka2 = a[keep], b[keep], a2[keep]
    assert same(got[0], i32(np.where(kb == 1, np.fix(100.0 / ka), -1)))
    assert same(got[1], i32(np.fix(100.0 / ka2)))
    bad = a2.copy(); bad[np.flatnonzero(keep)[11]] = 0                     # a kept zero behind the CASE
    with pytest.raises(dfgpu.DfgpuError, match="Divide by zero"):
        project(ctx, task_ctx, t.set_column(2, "a2", i32(bad)), exprs, predicate=C("keep", 3))
    bad = a.copy(); bad[np.flatnonzero(keep & (b == 1))[3]] = 0            # a kept row of the branch
    with pytest.raises(dfgpu.DfgpuError, match="Divide by zero"):
        project(ctx, task_ctx, t.set_column(0, "a", i32(bad)), exprs, predicate=C("keep", 3))


def test_boolean_case_as_filter_predicate(ctx, task_ctx):
    from dfgpu import physical_plan as ops
    C, B, L = ops.Column, ops.BinaryExpr, lambda v: ops.Literal(v, pa.int32())
    n = 3000
    rng = np.random.default_rng(37)
    x = pa.array(rng.integers(0, 100, n).astype(np.int32), mask=rng.random(n) < 0.1)
    y = pa.array(rng.integers(0, 100, n).astype(np.int32), mask=rng.random(n) < 0.1)
    pred = ops.CaseExpr(None, [(B(C("x", 0), "<", L(30)), B(C("y", 1), ">", L(50))), (B(C("x", 0), "<", L(60)), ops.Literal(True, pa.bool_()))], B(C("y", 1), "<", L(10)))
    got = project(ctx, task_ctx, pa.table({"x": x, "y": y, "row": pa.array(np.arange(n))}), [C("row", 2)], predicate=pred)
    lt = lambda col, v: [None if c is None else c < v for c in col.to_pylist()]
    gt = lambda col, v: [None if c is None else c > v for c in col.to_pylist()]
    mask = case_rows([lt(x, 30), lt(x, 60)], [gt(y, 50), [True] * n], lt(y, 10))
    assert got[0].to_pylist() == [i for i, m in enumerate(mask) if m is True]


def test_q12_shape_sum_of_case_grouped_by_dictionary(ctx, task_ctx):
    """TPC-H Q12: GROUP BY l_shipmode, SUM(CASE WHEN prio = '1-URGENT' OR prio = '2-HIGH' THEN 1 ELSE 0 END) and its complement -- the run-time compiled
    aggregate does not know the node, so the arguments are evaluated node by node"""
    from dfgpu import capi, physical_plan as ops
    C, B = ops.Column, ops.BinaryExpr
    n = 5000
    rng = np.random.default_rng(41)
    modes = np.array(["MAIL", "SHIP", "AIR", "RAIL"])[rng.integers(0, 4, n)]
    prios = np.array(["1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"])[rng.integers(0, 5, n)]
    t = pa.table({"shipmode": pa.array(modes).dictionary_encode(), "prio": pa.array(prios)})
    S = lambda v: ops.Literal(v, pa.utf8())
    I = lambda v: ops.Literal(v, pa.int64())
    high = B(B(C("prio", 1), "=", S("1-URGENT")), "OR", B(C("prio", 1), "=", S("2-HIGH")))
    low = B(B(C("prio", 1), "!=", S("1-URGENT")), "AND", B(C("prio", 1), "!=", S("2-HIGH")))
    aggs = [ops.AggregateFunctionExpr("SUM", ops.CaseExpr(None, [(high, I(1))], I(0)), "high_line_count", input_field=ops.Field("x", capi.INT64)),
            ops.AggregateFunctionExpr("SUM", ops.CaseExpr(None, [(low, I(1))], I(0)), "low_line_count", input_field=ops.Field("x", capi.INT64))]
    batch = ops.batch_from_arrow(ctx, t)
    plan = ops.AggregateExec("Single", [(C("shipmode", 0), "shipmode")], aggs, ops.MemoryExec([[batch]], batch.schema))
    out = pa.concat_tables([b.to_arrow() for b in ops.collect(plan, task_ctx)])
    got = {m: (h, l) for m, h, l in zip(plain(out.column(0).combine_chunks()).to_pylist(), out.column(1).to_pylist(), out.column(2).to_pylist())}
    is_high = np.isin(prios, ["1-URGENT", "2-HIGH"])
    assert got == {m: (int((is_high & (modes == m)).sum()), int((~is_high & (modes == m)).sum())) for m in np.unique(modes)}
