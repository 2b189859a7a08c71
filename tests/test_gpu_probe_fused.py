"""-m gpu: the bitmap probe with the scan filter folded in (dfgpu_join_probe_fused, FilterExec's pending predicate).
Kernel level: the fused entry point against "compare, then probe with the mask" through the existing entry points and against the CPU oracle's join over the
pre-filtered rows.  Plan level: the same plans with the ctx option "join_probe_fused_filter" 1 and 0.  Every comparison is exact (bits and index vectors, order
included)."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

OPS = {10: np.equal, 11: np.not_equal, 12: np.less, 13: np.less_equal, 14: np.greater, 15: np.greater_equal}       # DFGPU_OP_EQ .. DFGPU_OP_GTEQ
OP_AND = 20
PAIRS, DEFERRED, SELECTION = 0, 1, 2
LENGTHS = [0, 1, 511, 512, 513, (1 << 20) + 3]
NB = 30_000              # build keys 10, 13, .., unique and sorted: a rank index (bitmap over a range of 3 NB)


def build_keys(kt):
    return (np.arange(NB, dtype=np.int64) * 3 + 10).astype(kt)


def probe_keys(rng, pattern, n, kt):
    """sorted_dense: 512 consecutive rows inside one 64-word bitmap window (the window branch); random: every wave leaves it (the gather branch); outliers: sorted with
    ~1 % far keys (both branches inside one launch).  All three reach below key_min (10) and beyond the range."""
    lo, hi = -50, 3 * NB + 100
    if pattern == "random":
        k = rng.integers(lo, hi, n)
    else:
        k = np.sort(rng.integers(lo, hi, n))
        if pattern == "outliers" and n:
            far = rng.random(n) < 0.01
            k[far] = rng.integers(lo, hi, int(far.sum()))
    return k.astype(kt)


def scalar(ctx, v, pa_t):
    return ctx.from_arrow(pa.array([v], type=pa_t))


def check_fused(ctx, table, bk, k, pv, pa_pt, op, s, m, off=0):
    """fused pairs / selection of (keys k, predicate column pv, optional incoming mask m) against the two-step route and the oracle; `off`: the device arrays are zero-copy
    slices at that row offset of longer ones"""
    n = len(k)

    def dev(a, t=None):
        if not off:
            return ctx.from_arrow(pa.array(a, type=t))
        pad = np.zeros(off, dtype=a.dtype)
        return ctx.from_arrow(pa.array(np.concatenate([pad, a]), type=t)).slice(off, n)

    dk, dp = dev(k), dev(pv, pa_pt)
    dm = dev(m) if m is not None else None
    sc = scalar(ctx, s, pa_pt)
    fused = table.probe_fused([dk], dp, op, sc, mask=dm, form=PAIRS)
    assert fused is not None, "the rank-indexed table declined a predicate it is instantiated for"
    fb, fp = fused
    fsel = table.probe_fused([dk], dp, op, sc, mask=dm, form=SELECTION)
    fdb, fdp = table.probe_fused([dk], dp, op, sc, mask=dm, form=DEFERRED)
    # (1) compare, then probe with the mask
    cmp_mask = ctx.binary(op, dp, sc, rhs_scalar=True)
    if dm is not None:
        cmp_mask = ctx.binary(OP_AND, cmp_mask, dm)
    ub, up = table.probe([dk], mask=cmp_mask)
    usel = table.probe_selection([dk], mask=cmp_mask)
    assert np.array_equal(fp.to_numpy(), up.to_numpy()) and np.array_equal(fb.to_numpy(), ub.to_numpy())
    assert fsel is not None and usel is not None and len(fsel) == n
    assert np.array_equal(np.asarray(fsel.to_arrow()), np.asarray(usel.to_arrow())) if n else True
    udb, udp = table.probe_deferred([dk], mask=cmp_mask)                 # build rows left for later whenever there is a row to probe
    assert (fdb is None) == (udb is None) == (n > 0) and np.array_equal(fdp.to_numpy(), udp.to_numpy()) and np.array_equal(fdp.to_numpy(), up.to_numpy())
    # (2) the oracle's join over the pre-filtered rows
    keep = OPS[op](pv, s) & (m if m is not None else True)
    rows = np.nonzero(keep)[0]
    if len(rows):
        want = po.hash_join([[pa.array(bk)]], [[pa.array(k[rows])]], "Inner", batch_size=1 << 40)
        wp, wb = rows[want.probe_idx], want.build_idx
    else:
        wp = wb = np.zeros(0, dtype=np.int64)
    assert np.array_equal(fp.to_numpy().astype(np.int64), wp) and np.array_equal(fb.to_numpy().astype(np.int64), wb)
    if n:
        assert np.array_equal(np.nonzero(np.asarray(fsel.to_arrow()))[0], wp)
    return len(wp)


@pytest.mark.parametrize("has_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("pt", ["int32", "date32", "int64"])
@pytest.mark.parametrize("kt", [np.int32, np.int64], ids=["k32", "k64"])
def test_fused_probe_equals_compare_then_probe_and_the_oracle(ctx, kt, pt, has_mask):
    import dfgpu
    pa_pt = {"int32": pa.int32(), "date32": pa.date32(), "int64": pa.int64()}[pt]
    np_pt = np.int64 if pt == "int64" else np.int32
    rng = np.random.default_rng(7 + 3 * has_mask + len(pt))
    bk = build_keys(kt)
    table = dfgpu.JoinTable(ctx, [ctx.from_arrow(pa.array(bk))])
    matched = 0
    for n in LENGTHS:
        for pattern in ("sorted_dense", "random", "outliers"):
            k = probe_keys(rng, pattern, n, kt)
            pv = rng.integers(0, 100, n).astype(np_pt)
            m = (rng.random(n) < 0.6) if has_mask else None
            for op in OPS:
                matched += check_fused(ctx, table, bk, k, pv, pa_pt, op, 40, m)
    assert matched > 100_000


@pytest.mark.parametrize("kt", [np.int32, np.int64], ids=["k32", "k64"])
def test_fused_probe_edges(ctx, kt):
    """slices at an odd row offset (keys and predicate column are then not pair-aligned), predicate all-true and all-false, an empty build"""
    import dfgpu
    rng = np.random.default_rng(23)
    bk = build_keys(kt)
    table = dfgpu.JoinTable(ctx, [ctx.from_arrow(pa.array(bk))])
    for n in (513, 100_001):
        for pattern in ("sorted_dense", "random"):
            k = probe_keys(rng, pattern, n, kt)
            for np_pt, pa_pt in ((np.int32, pa.int32()), (np.int64, pa.int64())):
                pv = rng.integers(0, 100, n).astype(np_pt)
                m = rng.random(n) < 0.5
                for off in (1, 3):
                    assert check_fused(ctx, table, bk, k, pv, pa_pt, 12, 50, m, off=off) > 0
                    check_fused(ctx, table, bk, k, pv, pa_pt, 14, 50, None, off=off)
                assert check_fused(ctx, table, bk, k, pv, pa_pt, 15, 0, None) > 0          # all true
                assert check_fused(ctx, table, bk, k, pv, pa_pt, 12, 0, m) == 0            # all false
    # an empty build has no bitmap: the fused form declines before launching anything, the unfused probe answers with no pairs
    empty = dfgpu.JoinTable(ctx, [ctx.from_arrow(pa.array(np.zeros(0, dtype=kt)))])
    k = probe_keys(rng, "random", 1000, kt)
    dk, dp = ctx.from_arrow(pa.array(k)), ctx.from_arrow(pa.array(rng.integers(0, 100, 1000).astype(np.int32)))
    got = empty.probe_fused([dk], dp, 12, scalar(ctx, 50, pa.int32()))
    if got is not None:
        assert len(got[1]) == 0
    assert len(empty.probe([dk], mask=ctx.binary(12, dp, scalar(ctx, 50, pa.int32()), rhs_scalar=True))[1]) == 0


def test_fused_probe_declines_what_the_kernel_is_not_built_for(ctx):
    """Stated behaviour: a nullable key column, a nullable predicate column, a NULL scalar, an operator outside EQ..GTEQ, narrow keys and tables without a bitmap take the
    UNFUSED answer -- dfgpu_join_probe_fused returns DFGPU_NOT_IMPLEMENTED (None here) and launches nothing."""
    import dfgpu
    rng = np.random.default_rng(5)
    n = 20_000
    bk = build_keys(np.int64)
    table = dfgpu.JoinTable(ctx, [ctx.from_arrow(pa.array(bk))])
    k = probe_keys(rng, "random", n, np.int64)
    pv = rng.integers(0, 100, n).astype(np.int32)
    dk, dp, sc = ctx.from_arrow(pa.array(k)), ctx.from_arrow(pa.array(pv)), scalar(ctx, 40, pa.int32())
    nulls = rng.random(n) < 0.1
    t16 = dfgpu.JoinTable(ctx, [ctx.from_arrow(pa.array(np.arange(1000, dtype=np.int16)))])
    rep = dfgpu.JoinTable(ctx, [ctx.from_arrow(pa.array(rng.integers(0, 1 << 40, 5000).astype(np.int64)))])                 # sparse: hash table, no bitmap
    ctx.profile_select(None); ctx.profile_enable(True); ctx.profile_read()
    try:
        assert table.probe_fused([ctx.from_arrow(pa.array(k, mask=nulls))], dp, 12, sc) is None               # key validity
        assert table.probe_fused([dk], ctx.from_arrow(pa.array(pv, mask=nulls)), 12, sc) is None                # predicate validity
        assert table.probe_fused([dk], dp, 12, scalar(ctx, None, pa.int32())) is None                           # NULL scalar
        assert table.probe_fused([dk], dp, 16, sc) is None                                                      # IS DISTINCT FROM
        assert table.probe_fused([dk], dp, 12, scalar(ctx, 40, pa.int64())) is None                             # scalar of another type
        assert table.probe_fused([dk], ctx.from_arrow(pa.array(pv[:-1])), 12, sc) is None                       # lengths differ
        assert t16.probe_fused([ctx.from_arrow(pa.array(rng.integers(0, 2000, n).astype(np.int16)))], dp, 12, sc) is None      # narrow keys
        assert rep.probe_fused([dk], dp, 12, sc) is None
        launched = {name for name in ctx.profile_read() if not name.startswith("sync:")}
        assert not {"k_probe_match_bitmap", "k_probe_match_hash", "join_build_bitmap"} & launched, launched
        # the answer such a caller then gets: key validity through the unfused kernel
        keep = (pv < 40)
        ub, up = table.probe([ctx.from_arrow(pa.array(k, mask=nulls))], mask=ctx.from_arrow(pa.array(keep)))
        rows = np.nonzero(keep & ~nulls)[0]
        want = po.hash_join([[pa.array(bk)]], [[pa.array(k[rows])]], "Inner", batch_size=1 << 40)
        assert np.array_equal(up.to_numpy().astype(np.int64), rows[want.probe_idx]) and np.array_equal(ub.to_numpy().astype(np.int64), want.build_idx)
    finally:
        ctx.profile_enable(False)


# ----------------------------------------------------------------------------- plan level
class fused_filter:
    def __init__(self, ctx, on, metrics=0):
        self.ctx, self.on, self.metrics = ctx, on, metrics

    def __enter__(self):
        self.ctx.set_option("join_probe_fused_filter", self.on); self.ctx.set_option("collect_metrics", self.metrics)

    def __exit__(self, *a):
        self.ctx.set_option("join_probe_fused_filter", 1); self.ctx.set_option("collect_metrics", 0)


def profiled(ctx, fn):
    ctx.profile_select(None); ctx.profile_enable(True); ctx.profile_read()
    try:
        out = fn()
        return out, ctx.profile_read()
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("sf", [0.002, 0.02, 0.1])
def test_q3_fused_and_unfused_match_the_oracle(ctx, sf):
    """Q3 with the option on, off, and on with metrics collected: the oracle's rows each time and FilterExec's output_rows equal in all runs.  With device-sized batches
    (TaskContext batch_size 8192 < the table sizes from SF 0.02 on) the option decides whether the two date filters launch k_compare_scalar_fast at all; at SF 0.002 orders
    (3 000 rows) stays below the chunked bound, so its predicate goes through the resolver, and with batch_size 2^30 both do."""
    from dfgpu import physical_plan as ops, tpch
    from test_gpu_q3 import canon
    host = tpch.gen_host(sf)
    tables = tpch.upload(ctx, host)
    want = canon(po.tpch_q3(host, tpch.SEGMENTS.index(tpch.Q3_SEGMENT), tpch.Q3_DATE, target_partitions=4, batch_size=8192))

    def run(batch_size):
        plan = tpch.q3_plan(tables, batch_size=8192)
        tc = ops.TaskContext(ctx, batch_size=batch_size)
        got, prof = profiled(ctx, lambda: canon(tpch.q3_result_to_numpy(ops.collect(plan, tc))))
        assert len(got["l_orderkey"]) == len(want["l_orderkey"]) > 0
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        return plan, tc, prof.get("k_compare_scalar_fast", (0, 0.0))[0]

    filter_rows = lambda plan, tc: [m["output_rows"] for m in plan.metrics(tc) if m["name"] == "FilterExec"]
    with fused_filter(ctx, 1):
        _, _, cmp_on = run(8192)
    with fused_filter(ctx, 0):
        _, _, cmp_off = run(8192)
    with fused_filter(ctx, 1):
        _, _, cmp_resolved = run(1 << 30)
    assert cmp_off == 2 and cmp_resolved == 2
    assert cmp_on == (0 if sf >= 0.02 else 1)
    with fused_filter(ctx, 1, metrics=1):
        plan, tc, cmp_metered = run(8192)
        rows_on = filter_rows(plan, tc)
    with fused_filter(ctx, 0, metrics=1):
        plan, tc, _ = run(8192)
        rows_off = filter_rows(plan, tc)
    assert cmp_metered == 2                 # metrics count the filter's rows: the predicate is evaluated where it always was
    assert len(rows_on) == 3 and rows_on == rows_off
    assert sorted(rows_on) == sorted([int((host["c_mktsegment"] == tpch.SEGMENTS.index(tpch.Q3_SEGMENT)).sum()), int((host["o_orderdate"] < tpch.Q3_DATE).sum()),
                                      int((host["l_shipdate"] > tpch.Q3_DATE).sum())])


def _tables(rng, nullable=False):
    nb, npr = 20_000, 300_000
    build = pa.table({"b_key": pa.array(np.arange(nb, dtype=np.int64) * 2 + 5), "b_val": pa.array(rng.integers(0, 50, nb).astype(np.int32))})
    d = rng.integers(8000, 9000, npr).astype(np.int32)
    probe = pa.table({"p_key": pa.array(rng.integers(0, 2 * nb + 50, npr).astype(np.int64)), "p_date": pa.array(d, mask=(rng.random(npr) < 0.1) if nullable else None),
                      "p_val": pa.array(rng.integers(0, 1000, npr).astype(np.int64))})
    return build, probe


def _both(ctx, run):
    with fused_filter(ctx, 1):
        on, prof_on = profiled(ctx, run)
    with fused_filter(ctx, 0):
        off, prof_off = profiled(ctx, run)
    assert on.equals(off) and on.num_rows > 0
    return on, prof_on.get("k_compare_scalar_fast", (0, 0.0))[0], prof_off.get("k_compare_scalar_fast", (0, 0.0))[0]


@pytest.mark.parametrize("join_type", ["Inner", "Right", "Full", "RightSemi", "RightAnti"])
def test_filter_under_the_probe_side_of_every_join_type(ctx, task_ctx, join_type):
    """filter -> probe side: an Inner join takes the predicate into its probe (no compare launch); Right / Full / RightSemi / RightAnti emit unmatched probe rows, so the
    predicate is resolved first.  Rows and their order equal the option-off run and, for Inner, pyarrow's join over the filtered rows."""
    from dfgpu import physical_plan as ops
    C, L, B = ops.Column, ops.Literal, ops.BinaryExpr
    build, probe = _tables(np.random.default_rng(31))
    mk = lambda t: (lambda b: ops.MemoryExec([[b]], b.schema))(ops.batch_from_arrow(ctx, t))

    def run():
        f = ops.CoalesceBatchesExec(ops.FilterExec(B(L(8600, pa.int32()), ">", C("p_date", 1)), mk(probe)), 8192)          # literal on the left: p_date < 8600
        p = ops.ProjectionExec([(C("p_val", 2), "p_val"), (C("p_key", 0), "p_key")], f)                                       # drops the predicate's column
        j = ops.HashJoinExec(mk(build), p, [(C("b_key", 0), C("p_key", 1))], None, join_type, "CollectLeft")
        return pa.concat_tables([b.to_arrow() for b in j.execute(0, task_ctx)])

    on, cmp_on, cmp_off = _both(ctx, run)
    assert cmp_off == 1 and cmp_on == (0 if join_type == "Inner" else 1)
    if join_type == "Inner":
        kept = probe.filter(pc.less(probe["p_date"], 8600)).select(["p_val", "p_key"])
        want = kept.join(build, keys="p_key", right_keys="b_key", join_type="inner", coalesce_keys=False)
        rows = lambda t: sorted(zip(t["b_key"].to_pylist(), t["b_val"].to_pylist(), t["p_val"].to_pylist(), t["p_key"].to_pylist()))
        assert on.num_rows == want.num_rows and rows(on) == rows(want)


@pytest.mark.parametrize("shape", ["aggregate", "build_side", "nullable_column", "filter_above_filter", "filter_above_filter_projected"])
def test_filters_that_feed_something_else_behave_as_before(ctx, task_ctx, shape):
    """filter -> aggregate and filter -> join BUILD side are not marked (the compare runs with the option on and off); a filter on a nullable column is never deferred;
    of two stacked filters the upper one travels to the probe on top of the lower one's selection.  Results equal the option-off run."""
    import dfgpu
    from dfgpu import physical_plan as ops
    C, L, B = ops.Column, ops.Literal, ops.BinaryExpr
    build, probe = _tables(np.random.default_rng(37), nullable=shape == "nullable_column")
    mk = lambda t: (lambda b: ops.MemoryExec([[b]], b.schema))(ops.batch_from_arrow(ctx, t))
    cb = lambda p: ops.CoalesceBatchesExec(p, 8192)

    def run():
        if shape == "aggregate":
            f = cb(ops.FilterExec(B(C("p_date", 1), "<", L(8600, pa.int32())), mk(probe)))
            agg = ops.AggregateExec("Single", [(C("p_date", 1), "p_date")], [ops.AggregateFunctionExpr("SUM", C("p_val", 2), "s", input_field=ops.Field("p_val", dfgpu.capi.INT64))], f)
            t = pa.concat_tables([b.to_arrow() for b in agg.execute(0, task_ctx)])
            return t.sort_by("p_date")
        if shape == "build_side":           # the filtered table is the LEFT input
            f = cb(ops.FilterExec(B(C("p_date", 1), "<", L(8600, pa.int32())), mk(probe)))
            j = ops.HashJoinExec(f, mk(build), [(C("p_key", 0), C("b_key", 0))], None, "Inner", "CollectLeft")
        elif shape == "nullable_column":
            f = cb(ops.FilterExec(B(C("p_date", 1), "<", L(8600, pa.int32())), mk(probe)))
            j = ops.HashJoinExec(mk(build), f, [(C("b_key", 0), C("p_key", 0))], None, "Inner", "CollectLeft")
        else:
            f = cb(ops.FilterExec(B(C("p_val", 2), ">=", L(300, pa.int64())), mk(probe)))
            if shape == "filter_above_filter_projected":
                f = ops.ProjectionExec([(C("p_key", 0), "p_key"), (C("p_date", 1), "p_date"), (C("p_val", 2), "p_val")], f)
            f = cb(ops.FilterExec(B(C("p_date", 1), "<", L(8600, pa.int32())), f))
            j = ops.HashJoinExec(mk(build), f, [(C("b_key", 0), C("p_key", 0))], None, "Inner", "CollectLeft")
        return pa.concat_tables([b.to_arrow() for b in j.execute(0, task_ctx)])

    on, cmp_on, cmp_off = _both(ctx, run)
    if shape in ("aggregate", "build_side"):
        assert cmp_on == cmp_off == 1
    elif shape == "nullable_column":
        assert cmp_on == cmp_off == 0       # a nullable column never took the compare fast path either
    else:
        assert cmp_off == 2 and cmp_on == 1
        kept = probe.filter(pc.and_(pc.greater_equal(probe["p_val"], 300), pc.less(probe["p_date"], 8600)))
        assert on.num_rows == kept.join(build, keys="p_key", right_keys="b_key", join_type="inner").num_rows
