"""-m gpu: full-width Decimal128 arithmetic, aggregates and numeric casts against the exact reference (tests/exact_numeric.py).

Every value here may use the high 64 bits of the i128 payload: the 128-bit branch of mul128_checked (int128.h and the JIT prelude),
the long division of udivmod128, the carries of every SUM kernel and of the partitioned pre-aggregation, the two-pass Decimal128
MIN / MAX.  Results are compared with plain Python integers, not with the C oracle or the node-by-node device path, so a mistake those
share cannot pass.  Each check covers value, type and NULLs, and an error must be raised exactly when the reference raises one.
Float scales stay at 22 or below: 10^s is exact in an f64 only up to 10^22, beyond that `powi` and a multiplication loop may differ."""
import math
import zlib

import numpy as np
import pyarrow as pa
import pytest

import exact_numeric as E
from test_exact_numeric import CMP_OPS, DEC_BINARY_TYPES, binary_inputs, cast_cases, cast_check

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(31337)
OPCODE = {"+": 0, "-": 1, "*": 2, "/": 3, "%": 4, "=": 10, "!=": 11, "<": 12, "<=": 13, ">": 14, ">=": 15}
KIND = {"SUM": 0, "AVG": 1, "COUNT": 2, "MIN": 3, "MAX": 4}


def _err():
    import dfgpu
    return dfgpu.DfgpuError


def dev_binary(ctx, op, xs, ys, t1, t2, ls=False, rs=False):
    def run(rows):
        l = E.make_column(t1, xs if ls else [xs[i] for i in rows])
        r = E.make_column(t2, ys if rs else [ys[i] for i in rows])
        return ctx.binary(OPCODE[op], ctx.from_arrow(l), ctx.from_arrow(r), ls, rs).to_arrow()
    return run


# ------------------------------------------------------------------------------------------------------------- binary arithmetic
@pytest.mark.parametrize("op", ["+", "-", "*", "/", "%"])
@pytest.mark.parametrize("types", DEC_BINARY_TYPES, ids=[f"{a}x{b}" for a, b in DEC_BINARY_TYPES])
def test_decimal_binary_full_width(ctx, op, types):
    t1, t2 = pa.decimal128(*types[0]), pa.decimal128(*types[1])
    xs, ys = binary_inputs(t1, t2)
    p, s, lm, rm = E.decimal_binary_plan(op, t1.precision, t1.scale, t2.precision, t2.scale)
    exp = E.expect_rows(lambda i: None if xs[i] is None or ys[i] is None else E.decimal_binary_value(op, xs[i], ys[i], lm, rm), len(xs))
    n_ok, n_err = E.check_rows(dev_binary(ctx, op, xs, ys, t1, t2), exp, pa.decimal128(p, s), _err(), label=f"{t1} {op} {t2}")
    assert n_ok > len(xs) // 4
    if op in "+-":       # arrow checks the i128 payload, not the precision: results above 10^38 that fit i128 are no error
        assert any(isinstance(v, int) and abs(v) >= 10 ** 38 for v in exp)
    for sc in (E.I128_MIN + 1, -1, 0, (1 << 64) + 1, 10 ** 19):
        exp = E.expect_rows(lambda i: None if ys[i] is None else E.decimal_binary_value(op, sc, ys[i], lm, rm), len(ys))
        E.check_rows(dev_binary(ctx, op, [sc], ys, t1, t2, ls=True), exp, pa.decimal128(p, s), _err(), max_error_rows=8, label=f"{sc} {op} column")
        exp = E.expect_rows(lambda i: None if xs[i] is None else E.decimal_binary_value(op, xs[i], sc, lm, rm), len(xs))
        E.check_rows(dev_binary(ctx, op, xs, [sc], t1, t2, rs=True), exp, pa.decimal128(p, s), _err(), max_error_rows=8, label=f"column {op} {sc}")


def test_decimal_multiply_scale_39_fails(ctx):
    t1, t2 = pa.decimal128(38, 20), pa.decimal128(38, 19)
    with pytest.raises(_err()):
        dev_binary(ctx, "*", [1, 2], [1, 2], t1, t2)([0, 1])


@pytest.mark.parametrize("op", ["/", "%"])
def test_decimal_i128_min_by_minus_one_overflows(ctx, op):
    t1 = pa.decimal128(38, 38) if op == "/" else pa.decimal128(38, 0)         # the only types whose dividend is not rescaled
    t2 = pa.decimal128(38, 0)
    xs = [E.I128_MIN, E.I128_MIN, E.I128_MIN + 1, E.I128_MIN + 1, E.I128_MAX, E.I128_MIN, E.I128_MIN, -(1 << 64)]
    ys = [-1, 1, -1, 1, -1, 2, E.I128_MAX, -1]
    p, s, lm, rm = E.decimal_binary_plan(op, t1.precision, t1.scale, t2.precision, t2.scale)
    exp = E.expect_rows(lambda i: E.decimal_binary_value(op, xs[i], ys[i], lm, rm), len(xs))
    E.check_rows(dev_binary(ctx, op, xs, ys, t1, t2), exp, pa.decimal128(p, s), _err())


@pytest.mark.parametrize("op", list(CMP_OPS))
def test_decimal_comparisons_full_width(ctx, op):
    """same scale, every pair of edge values: pairs that differ only in the low word (an unsigned low-word compare) in both signs"""
    t = pa.decimal128(38, 6)
    e = E.edge_table(38)
    xs = [x for x in e for _ in e] + [None, 1]
    ys = [y for _ in e for y in e] + [1, None]
    got = ctx.binary(OPCODE[op], ctx.from_arrow(E.make_column(t, xs)), ctx.from_arrow(E.make_column(t, ys))).to_arrow()
    assert got.to_pylist() == [None if x is None or y is None else CMP_OPS[op](x, y) for x, y in zip(xs, ys)]
    sc = (5 << 64) | 1
    got = ctx.binary(OPCODE[op], ctx.from_arrow(E.make_column(t, xs)), ctx.from_arrow(E.make_column(t, [sc])), False, True).to_arrow()
    assert got.to_pylist() == [None if x is None else CMP_OPS[op](x, sc) for x in xs]


# ------------------------------------------------------------------------------------------------- fused x op (literal op y)
SHAPES = {"x*(1-y)": ("*", "-", True, False), "(1+y)*x": ("*", "+", True, True), "x-(y/2)": ("-", "/", False, False), "(y-1)/x": ("/", "-", False, True)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_two_level_arithmetic_full_width(ctx, task_ctx, shape):
    """ProjectionExec of `x op (lit op2 y)` runs as one fused pass: at full width its values must be exact, one overflowing row must fail
    the projection with the node-by-node error kind, and the same row dropped by a selection first must not."""
    import dfgpu
    from dfgpu import physical_plan as ops
    outer, inner, lit_left, inner_left = SHAPES[shape]
    tx, ty, tl = pa.decimal128(38, 2), pa.decimal128(30, 2), pa.decimal128(20, 0)
    lit = 1 if shape != "x-(y/2)" else 2
    n = 3000
    xs = [v if v != 0 else 7 for v in E.random_values(RNG, n, 19)] + [(1 << 64) + 3, -(1 << 64) - 3, 10 ** 20 + 1, E.U64]
    ys = [v if v != 0 else 3 for v in E.random_values(RNG, n, 17)] + [(1 << 63) + 5, -(1 << 63), 10 ** 16, 1]
    pi, si, lmi, rmi = E.decimal_binary_plan(inner, *((tl.precision, tl.scale, ty.precision, ty.scale) if lit_left else (ty.precision, ty.scale, tl.precision, tl.scale)))
    ti = pa.decimal128(pi, si)
    po_, so, lmo, rmo = E.decimal_binary_plan(outer, *((pi, si, tx.precision, tx.scale) if inner_left else (tx.precision, tx.scale, pi, si)))
    lit_u = lit * 10 ** tl.scale

    def exact(x, y):
        t = E.decimal_binary_value(inner, lit_u, y, lmi, rmi) if lit_left else E.decimal_binary_value(inner, y, lit_u, lmi, rmi)
        return E.decimal_binary_value(outer, t, x, lmo, rmo) if inner_left else E.decimal_binary_value(outer, x, t, lmo, rmo)

    C, B = ops.Column, ops.BinaryExpr
    lit_e = ops.Literal(__import__("decimal").Decimal(lit), tl)
    inner_e = B(lit_e, inner, C("y", 1)) if lit_left else B(C("y", 1), inner, lit_e)
    expr = B(inner_e, outer, C("x", 0)) if inner_left else B(C("x", 0), outer, inner_e)

    def project(xv, yv, keep=None):
        t = pa.table({"x": E.make_column(tx, xv), "y": E.make_column(ty, yv), "keep": pa.array(keep if keep is not None else [True] * len(xv))})
        b = ops.batch_from_arrow(ctx, t)
        src = ops.MemoryExec([[b]], b.schema)
        if keep is not None:
            src = ops.FilterExec(C("keep", 2), src)
        out = ops.collect(ops.ProjectionExec([(expr, "e")], src), task_ctx)
        return pa.concat_arrays([o.columns[0].to_arrow() for o in out])

    exp = E.expect_rows(lambda i: exact(xs[i], ys[i]), len(xs))
    ok = [i for i in range(len(xs)) if not isinstance(exp[i], type)]
    got = project([xs[i] for i in ok], [ys[i] for i in ok])
    assert got.type == pa.decimal128(po_, so)
    assert E.decimal_values(got) == [exp[i] for i in ok]
    assert any(abs(exp[i]) >= 1 << 64 for i in ok)
    # one row that overflows in the outer operation: the product; x rescaled by 10^4 for the difference; (y - 1) rescaled by 10^6 for the quotient
    big_x, big_y = {"*": (10 ** 37, 10 ** 27), "-": (10 ** 37, 1), "/": (10 ** 36, 10 ** 33)}[outer]
    bx, by = xs[:200] + [big_x], ys[:200] + [big_y]
    bad = E.expect_rows(lambda i: exact(bx[i], by[i]), len(bx))
    kinds = {E.ERROR_KIND[b] for b in bad if isinstance(b, type)}
    assert kinds, "the test must plant an overflowing row"
    with pytest.raises(dfgpu.DfgpuError) as e:
        project(bx, by)
    assert E.error_kind(e.value) in kinds
    keep = [not isinstance(b, type) for b in bad]
    got = project(bx, by, keep)
    assert E.decimal_values(got) == [b for b in bad if not isinstance(b, type)]


# ------------------------------------------------------------------------------------------------------- fused aggregate (JIT)
@pytest.mark.parametrize("masked", [False, True])
def test_update_batch_fused_full_width(ctx, masked):
    """SUM(x * (1 - y)) and SUM(x) through the run-time compiled kernel, x up to ~10^30: the 128-bit branch of the prelude's
    mul128_checked and the carry of the generated 128-bit add.  Compared with the exact sums, not with the node-by-node path."""
    import dfgpu
    n, total = 40000, 7                                                    # the fused kernel keeps its partials in registers: <= 8 groups
    tx, ty, tl = pa.decimal128(38, 2), pa.decimal128(15, 2), pa.decimal128(20, 0)
    r = np.random.default_rng(5)
    xs = [int(v) * (10 ** int(k)) + int(w) for v, k, w in zip(r.integers(-10 ** 15, 10 ** 15, n), r.integers(0, 16, n), r.integers(0, 1 << 62, n))]
    xs[:4] = [(1 << 64) - 1, 1 << 64, -(1 << 64), 10 ** 30 - 1]
    ys = r.integers(0, 11, n).tolist()
    gids = r.integers(0, total, n)
    keep = r.random(n) < 0.7 if masked else np.ones(n, dtype=bool)
    cols = [ctx.from_arrow(E.make_column(tx, xs)), ctx.from_arrow(E.make_column(ty, ys)), ctx.from_arrow(E.make_column(tl, [1]))]
    nodes = [("column", 0, 0), ("column", 1, 0), ("scalar", 2, 0), ("-", 2, 1), ("*", 0, 3)]
    prod_t = pa.decimal128(38, 4)
    accs = [dfgpu.GroupsAccumulator(ctx, KIND["SUM"], dfgpu.capi.DECIMAL128, prod_t.precision, prod_t.scale),
            dfgpu.GroupsAccumulator(ctx, KIND["SUM"], dfgpu.capi.DECIMAL128, tx.precision, tx.scale)]
    g = ctx.from_arrow(pa.array(gids.astype(np.uint32)))
    filt = ctx.from_arrow(pa.array(keep)) if masked else None
    dfgpu.GroupsAccumulator.update_batch_fused(ctx, accs, [4, 0], nodes, cols, g, filt, total)
    prods = [x * (100 - y) for x, y in zip(xs, ys)]                     # (scale 2) * (1.00 - y/100 at scale 2) at scale 4
    kept = keep.tolist()
    want_p = E.group_sums([p if k else None for p, k in zip(prods, kept)], gids.tolist(), total)[0]
    want_x = E.group_sums([x if k else None for x, k in zip(xs, kept)], gids.tolist(), total)[0]
    got_p, got_x = accs[0].evaluate().to_arrow(), accs[1].evaluate().to_arrow()
    assert got_p.type == E.sum_type(prod_t) and got_x.type == E.sum_type(tx)
    assert E.decimal_values(got_p) == want_p
    assert E.decimal_values(got_x) == want_x
    assert any(abs(v) >= 1 << 64 for v in want_p)


# ------------------------------------------------------------------------------------------------------------------ accumulators
def dev_acc(ctx, kind, t, batches, total, multi=False):
    """batches: [(values, gids, keep or None)] -> the evaluated device array (raises DfgpuError from evaluate)"""
    import dfgpu
    acc = dfgpu.GroupsAccumulator(ctx, KIND[kind], dfgpu.capi.DECIMAL128, t.precision, t.scale)
    for vals, gids, keep in batches:
        v = ctx.from_arrow(E.make_column(t, vals))
        g = ctx.from_arrow(pa.array(np.asarray(gids, dtype=np.uint32)))
        f = ctx.from_arrow(pa.array(keep)) if keep is not None else None
        if multi:
            dfgpu.GroupsAccumulator.update_batch_multi(ctx, [acc], [v], [f], g, total)
        else:
            acc.update_batch(v, g, f, total)
    return acc


def exact_acc(kind, t, batches, total):
    vals, gids = [], []
    for v, g, keep in batches:
        vals += [x if keep is None or keep[i] else None for i, x in enumerate(v)]
        gids += list(np.asarray(g).tolist())
    if kind == "SUM":
        return E.group_sums(vals, gids, total)[0]
    if kind == "AVG":
        return E.group_avgs(vals, gids, total, t)
    return E.group_minmax(vals, gids, total, kind == "MIN")


def check_acc(ctx, kind, t, batches, total, multi=False):
    acc = dev_acc(ctx, kind, t, batches, total, multi)
    got = acc.evaluate().to_arrow()
    want = exact_acc(kind, t, batches, total)
    assert got.type == (E.sum_type(t) if kind == "SUM" else E.avg_type(t) if kind == "AVG" else t)
    gv = E.decimal_values(got)
    bad = [(g, w, v) for g, (w, v) in enumerate(zip(want, gv)) if w != v]
    assert not bad, f"{kind} {t}: {len(bad)} of {total} groups differ, first (group, expected, got): {bad[:3]}"
    return acc


def values_for(kind, t, n, r):
    """SUM / MIN / MAX: full width (sums wrap past 2^127 by add_wrapping); AVG: below 10^29, so that even a group of all 120 000 rows
    keeps sum * 10^4 inside i128 (the overflow has a test of its own)"""
    return E.random_values(r, n, min(t.precision, 29) if kind == "AVG" else t.precision)


BRANCHES = [  # (branch, kinds, rows, groups, filter, nulls, skew)
    ("k_acc_small", ("SUM", "AVG"), 60000, 6, False, False, False),
    ("k_acc_small_filtered_nulls", ("SUM", "AVG"), 60000, 8, True, True, False),
    ("k_acc_cached_plain", ("SUM", "AVG"), 120000, 1500, False, False, True),
    ("k_acc_cached_nulls", ("SUM", "AVG"), 120000, 1500, True, True, True),
    ("k_acc_add_plain", ("SUM", "AVG"), 50000, 20000, False, False, False),
    ("k_acc_update_add_filter", ("SUM", "AVG"), 50000, 20000, True, False, False),
    ("k_acc_update_add_nulls", ("SUM", "AVG"), 50000, 20000, False, True, False),
    ("k_acc_update_minmax128_few", ("MIN", "MAX"), 60000, 5, False, True, False),
    ("k_acc_update_minmax128_cached_shape", ("MIN", "MAX"), 120000, 1500, True, False, True),
    ("k_acc_update_minmax128_many", ("MIN", "MAX"), 50000, 20000, False, False, False),
]


@pytest.mark.parametrize("p,s", [(38, 4), (18, 2)])
@pytest.mark.parametrize("branch", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_accumulator_branch_full_width(ctx, branch, p, s):
    _, kinds, n, total, filt, nulls, skew = branch
    t = pa.decimal128(p, s)
    r = np.random.default_rng(zlib.crc32(f"{branch[0]}-{p}".encode()))
    gids = (np.minimum(r.zipf(1.3, n) - 1, total - 1) if skew else r.integers(0, total, n)).astype(np.int64)
    keep = (r.random(n) < 0.8).tolist() if filt else None
    for kind in kinds:
        vals = values_for(kind, t, n, r)
        if nulls:
            vals = [None if m else v for v, m in zip(vals, (r.random(n) < 0.1).tolist())]
        check_acc(ctx, kind, t, [(vals, gids, keep)], total)


@pytest.mark.parametrize("p,s", [(38, 0), (18, 0)])
@pytest.mark.parametrize("groups", [4, 2000, 30000], ids=["small", "cached", "add"])
def test_sum_crosses_two_words_from_positive_and_negative_terms(ctx, groups, p, s):
    """terms just under the precision limit, all positive, then all negative: each group's sum passes 2^64 (or -2^64); at (38, 0) the
    positive sums also wrap past 2^127 and must equal add_wrapping, with no error"""
    t = pa.decimal128(p, s)
    n = 60000 if groups > 2000 else 120000
    r = np.random.default_rng(groups + p)
    gids = r.integers(0, groups, n)
    top = 10 ** p - 1
    for sign in (1, -1):
        vals = [sign * (top - int(d)) for d in r.integers(0, 1000, n)]
        check_acc(ctx, "SUM", t, [(vals, gids, None)], groups)
        if groups <= 2000:                                                   # >= 30 terms of ~10^18 per group: past 2^64 everywhere
            raw = [0] * groups
            for v, g in zip(vals, gids.tolist()):
                raw[g] += v
            assert all(abs(x) >= 1 << 64 for x in raw)
    if p == 38:
        big = [E.I128_MAX - int(d) for d in r.integers(0, 10 ** 6, n)]          # the payload's limit, not the precision's: wraps past 2^127
        check_acc(ctx, "SUM", t, [(big, gids, None)], groups)


@pytest.mark.parametrize("groups", [5, 1500, 30000])
def test_minmax_extreme_changes_high_word_across_batches(ctx, groups):
    """three batches whose values take a few high words and adversarial low words (0, 1, 2^63, 2^64-1): a group's MAX moves to a higher
    and its MIN to a lower high word in a later batch, where the stale low word of the old extreme would win a low-word compare"""
    t = pa.decimal128(38, 0)
    r = np.random.default_rng(groups)
    los = [0, 1, 1 << 63, E.U64]
    batches = []
    for b, his in enumerate(([-1, 0, 1], [-2, 2, 0, 1], [-3, -1, 3, 2])):
        n = 3 * groups + 500
        g = r.integers(0, groups, n)
        hs = r.choice(his, n).tolist()
        ls = r.choice(len(los), n).tolist()
        vals = [h * (1 << 64) + los[li] for h, li in zip(hs, ls)]             # high word h, low word los[li]
        batches.append((vals, g, None))
    for kind in ("MIN", "MAX"):
        for k in range(1, 4):
            check_acc(ctx, kind, t, batches[:k], groups)


@pytest.mark.parametrize("p", [38, 18])
def test_merge_and_update_multi_full_width(ctx, p):
    """state() of one accumulator merged into another under a permutation of group ids, and update_batch_multi over the same batch"""
    import dfgpu
    t = pa.decimal128(p, 3)
    n, total = 40000, 3000
    r = np.random.default_rng(p)
    gids = r.integers(0, total, n)
    for kind in ("SUM", "AVG", "MIN", "MAX"):
        vals = values_for(kind, t, n, r)
        a = check_acc(ctx, kind, t, [(vals, gids, None)], total, multi=True)
        perm = r.permutation(total)
        b = dfgpu.GroupsAccumulator(ctx, KIND[kind], dfgpu.capi.DECIMAL128, t.precision, t.scale)
        b.merge_batch(a.state(), ctx.from_arrow(pa.array(perm.astype(np.uint32))), None, total)
        b.merge_batch(a.state(), ctx.from_arrow(pa.array(perm.astype(np.uint32))), None, total)        # twice: the sums double
        want = exact_acc(kind, t, [(vals, gids, None)] * 2, total)
        got = E.decimal_values(b.evaluate().to_arrow())
        inv = [None] * total
        for src, dst in enumerate(perm.tolist()):
            inv[dst] = want[src]
        assert got == inv, kind


@pytest.mark.parametrize("p", [38, 18])
def test_avg_overflow_and_negative_truncation(ctx, p):
    """AVG of negative sums truncates toward zero; a sum whose 10^4 rescale overflows i128 raises 'Arithmetic Overflow in AvgAccumulator'"""
    import dfgpu
    t = pa.decimal128(p, 2)
    gids = [0, 0, 0, 1, 1, 2, 3, 3, 3]
    lim = 10 ** min(p, 30)                                                 # sum * 10^4 in i128: the overflow comes below
    vals = [-1, -1, -2, -7, 0, -(lim // 10) - 1, -(lim - 1), -(lim - 2), -1]
    check_acc(ctx, "AVG", t, [(vals, gids, None)], 4)
    if p == 38:
        big = [10 ** 35, 10 ** 35, 5]                                      # 2 * 10^35 * 10^4 > 2^127; the sum itself fits
        acc = dev_acc(ctx, "AVG", t, [(big, [0, 0, 1], None)], 2)
        with pytest.raises(dfgpu.DfgpuError) as e:
            acc.evaluate()
        assert "AvgAccumulator" in str(e.value)
        with pytest.raises(E.ArithmeticOverflow):
            E.group_avgs(big, [0, 0, 1], 2, t)


# ------------------------------------------------------------------------------------------------- partitioned pre-aggregation
def pagg_run(ctx, keys, aggs, t):
    import dfgpu
    from test_gpu_pagg import forced
    kd = ctx.from_arrow(pa.array(keys))
    vd = [ctx.from_arrow(E.make_column(t, v)) for _, v in aggs]
    with forced(ctx) as f:
        pk, states = dfgpu.agg_preaggregate(ctx, kd, [KIND[k] for k, _ in aggs], vd)
        ran = f.kernels()
    assert "pa_aggregate" in ran, ran
    gv = dfgpu.GroupValues(ctx, 1)
    g = gv.intern([pk])
    out = []
    for (k, _), st in zip(aggs, states):
        acc = dfgpu.GroupsAccumulator(ctx, KIND[k], dfgpu.capi.DECIMAL128, t.precision, t.scale)
        acc.merge_batch(st, g, None, len(gv))
        out.append(acc.evaluate().to_arrow())
    return gv.emit()[0].to_arrow().to_pylist(), out


@pytest.mark.parametrize("case", ["38-full-width", "18-positive-near-limit", "18-negative-near-limit"])
def test_partitioned_preaggregation_full_width(ctx, case):
    """SUM / AVG through pa_aggregate: Decimal128(38, s) with both signs at full width (the PA_SUM_I128_HI cell), and Decimal128(18, s)
    with terms near 10^18 - 1 whose group totals pass 2^64 (or -2^64) through the sign-extended PA_SUM_I128_SX cell's carry"""
    n = 200000
    r = np.random.default_rng(len(case))
    if case.startswith("38"):
        t, groups = pa.decimal128(38, 4), 20000
        sums = E.random_values(r, n, 38)
        avgs = values_for("AVG", t, n, r)
        aggs = [("SUM", sums), ("AVG", avgs)]
    else:
        t, groups = pa.decimal128(18, 2), 60
        sign = 1 if "positive" in case else -1
        v = [sign * (10 ** 18 - 1 - int(d)) for d in r.integers(0, 10 ** 6, n)]
        aggs = [("SUM", v), ("AVG", v)]
    keys = (r.integers(0, groups, n) * 7919 + 11).astype(np.int64)
    got_keys, got = pagg_run(ctx, keys, aggs, t)
    kid = {k: i for i, k in enumerate(got_keys)}
    assert len(kid) == len(set(keys.tolist()))
    gids = [kid[k] for k in keys.tolist()]
    for (kind, vals), arr in zip(aggs, got):
        want = E.group_sums(vals, gids, len(kid))[0] if kind == "SUM" else E.group_avgs(vals, gids, len(kid), t)
        assert arr.type == (E.sum_type(t) if kind == "SUM" else E.avg_type(t))
        assert E.decimal_values(arr) == want, kind
        if not case.startswith("38") and kind == "SUM":
            assert all(abs(w) >= 1 << 64 for w in want)


def test_partitioned_preaggregation_declines_decimal_minmax(ctx):
    import dfgpu
    from test_gpu_pagg import forced
    n = 100000
    t = pa.decimal128(38, 2)
    kd = ctx.from_arrow(pa.array(RNG.integers(0, 5000, n).astype(np.int64)))
    vd = ctx.from_arrow(E.make_column(t, E.random_values(RNG, n, 38)))
    with forced(ctx):
        for kind in ("MIN", "MAX"):
            with pytest.raises(dfgpu.DfgpuError) as e:
                dfgpu.agg_preaggregate(ctx, kd, [KIND["SUM"], KIND[kind]], [vd, vd])
            assert e.value.kind == "NotImplemented"


# ----------------------------------------------------------------------------------------------------------------------------- casts
def dev_cast(ctx):
    import dfgpu
    from dfgpu import capi
    code = {pa.int8(): capi.INT8, pa.int16(): capi.INT16, pa.int32(): capi.INT32, pa.int64(): capi.INT64, pa.uint8(): capi.UINT8,
            pa.uint16(): capi.UINT16, pa.uint32(): capi.UINT32, pa.uint64(): capi.UINT64, pa.float32(): capi.FLOAT32, pa.float64(): capi.FLOAT64}

    def run(arr, dst):
        if pa.types.is_decimal(dst):
            return ctx.cast(ctx.from_arrow(arr), dfgpu.capi.DECIMAL128, dst.precision, dst.scale).to_arrow()
        return ctx.cast(ctx.from_arrow(arr), code[dst]).to_arrow()
    return run


@pytest.mark.parametrize("src,dst", cast_cases(), ids=[f"{s}->{t}" for s, t in cast_cases()])
def test_cast_equals_exact(ctx, src, dst):
    cast_check(dev_cast(ctx), src, dst, _err(), 24)


CAST_DEFECTS = [  # (defect, source type, value, target type, exact result or None for an error)
    ("1-decimal128-to-f64-rounds-once", pa.decimal128(38, 0), 27670116110564333567, pa.float64(), 27670116110564331520.0),
    ("1-decimal128-to-f64-negative", pa.decimal128(38, 0), -27670116110564333567, pa.float64(), -27670116110564331520.0),
    ("1-decimal128-to-f32-via-f64", pa.decimal128(38, 0), 27670116110564333567, pa.float32(), float(np.float32(27670116110564331520.0))),
    ("2-uint64-to-f64-rounds-once", pa.uint64(), 9223372036854778879, pa.float64(), 9223372036854777856.0),
    ("3-int64-to-f32-rounds-once", pa.int64(), 4611686843061108735, pa.float32(), 4611686568183201792.0),
    ("3-uint64-to-f32-rounds-once", pa.uint64(), 9223373686122217471, pa.float32(), 9223373136366403584.0),
    ("4-f64-below-int64-min", pa.float64(), -9.25e18, pa.int64(), None),
    ("4-f64-at-int64-min", pa.float64(), -(2.0 ** 63), pa.int64(), -(1 << 63)),
    ("4-f64-at-2^64-to-uint64", pa.float64(), 2.0 ** 64, pa.uint64(), None),
    ("4-f64-above-2^64-to-uint64", pa.float64(), 1.84467440737095537e19, pa.uint64(), None),
    ("4-f64-below-2^64-to-uint64", pa.float64(), math.nextafter(2.0 ** 64, 0), pa.uint64(), int(math.nextafter(2.0 ** 64, 0))),
]


@pytest.mark.parametrize("defect", CAST_DEFECTS, ids=[d[0] for d in CAST_DEFECTS])
def test_cast_predicted_defects(ctx, defect):
    _, src, v, dst, want = defect
    try:
        ref = E.cast_value(v, src, dst)
    except E.CastError:
        ref = None
    assert ref == want
    arr = E.make_column(src, [v])
    if want is None:
        with pytest.raises(_err()):
            dev_cast(ctx)(arr, dst)
    else:
        got = dev_cast(ctx)(arr, dst)
        assert got.type == dst and E.column_values(got) == [want]
