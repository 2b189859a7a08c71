"""HashJoinExec with and without a JoinFilter, all eight join types, on both output routes of the plan layer (chunks of batch_size pairs for
reference-sized probe batches, one piece for larger ones) and with an empty build or probe input, against the CPU oracle.  Plus: the three join
constructors refuse a JoinFilter whose column-index arrays are null."""
import ctypes as C
import functools

import numpy as np
import pyarrow as pa
import pytest

from helpers import rows_of, sort_rows
from oracle import pyoracle as po

JOIN_TYPES = ["Inner", "Left", "Right", "Full", "LeftSemi", "RightSemi", "LeftAnti", "RightAnti"]
SHAPES = {              # shape -> (build batch sizes, probe batch sizes, batch_size)
    "chunked": ((300, 1, 500), (700, 64, 200), 1024),        # probe batches of at most max(batch_size, 8192) rows: answered in chunks of batch_size pairs
    "whole": ((300, 1, 500), (9000,), 8192),                 # one probe batch of more rows than that: answered in one piece
    "empty_build": ((0,), (700, 64, 200), 1024),
    "empty_probe": ((300, 1, 500), (0,), 1024),
}


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(build tables, probe tables): k = key (50 / 70 distinct values, 10 % NULL), v / w = payload in 0 .. 1000, w 10 % NULL."""
    rng = np.random.default_rng(20241)
    bsizes, psizes, _ = SHAPES[shape]
    lb = [pa.table({"k": pa.array(rng.integers(0, 50, n).astype(np.int64), mask=rng.random(n) < 0.1), "v": pa.array(rng.integers(0, 1001, n).astype(np.int64))}) for n in bsizes]
    rb = [pa.table({"k": pa.array(rng.integers(0, 70, n).astype(np.int64), mask=rng.random(n) < 0.1),
                    "w": pa.array(rng.integers(0, 1001, n).astype(np.int64), mask=rng.random(n) < 0.1)}) for n in psizes]
    return lb, rb


def expected_rows(jt, with_filter, shape):
    """The oracle's rows in its order, and how many key-matched pairs the filter saw and kept."""
    lb, rb = inputs(shape)
    batch_size = SHAPES[shape][2]
    lcat = pa.concat_tables(lb[::-1])              # the oracle's build index points into the reversed concatenation of the build batches
    lk, lv = lcat["k"].to_pylist(), lcat["v"].to_pylist()
    lv_np = lcat["v"].to_numpy()
    rk = [t["k"].to_pylist() for t in rb]; rw = [t["w"].to_pylist() for t in rb]
    rw_np = [t["w"].combine_chunks().fill_null(0).to_numpy() for t in rb]; rw_ok = [~np.asarray(t["w"].combine_chunks().is_null()) for t in rb]
    seen = kept = 0

    def fn(pb, bi, pi):
        nonlocal seen, kept
        keep = rw_ok[pb][pi] & (lv_np[bi] > rw_np[pb][pi])
        seen += len(keep); kept += int(keep.sum())
        return keep.astype(np.uint8)

    res = po.hash_join([[t["k"]] for t in lb], [[t["k"]] for t in rb], jt, batch_size=batch_size, filter_fn=fn if with_filter else None)
    want = []
    for bi, pi, pb in zip(res.build_idx.tolist(), res.probe_idx.tolist(), res.probe_batch.tolist()):
        l = [None, None] if bi < 0 else [lk[bi], lv[bi]]
        r = [None, None] if pi < 0 else [rk[pb][pi], rw[pb][pi]]
        want.append(l if jt in ("LeftSemi", "LeftAnti") else r if jt in ("RightSemi", "RightAnti") else l + r)
    return want, seen, kept


def case_problems(ctx, jt, with_filter, shape):
    """What is wrong with one case, as a list of messages (empty: nothing)."""
    import dfgpu
    from dfgpu import physical_plan as ops
    lb, rb = inputs(shape)
    batch_size = SHAPES[shape][2]
    mk = lambda tabs: ops.MemoryExec([[ops.batch_from_arrow(ctx, t) for t in tabs]], ops.batch_from_arrow(ctx, tabs[0]).schema)
    filt = None
    if with_filter:
        filt = ops.JoinFilter(ops.BinaryExpr(ops.Column("x", 0), ">", ops.Column("y", 1)), [("left", 1), ("right", 1)],
                              ops.Schema([ops.Field("x", dfgpu.capi.INT64), ops.Field("y", dfgpu.capi.INT64)]))
    join = ops.HashJoinExec(mk(lb), mk(rb), [(ops.Column("k", 0), ops.Column("k", 0))], filt, jt, "CollectLeft")
    got = []
    for b in ops.collect(join, ops.TaskContext(ctx, batch_size=batch_size)):
        got += rows_of([c.to_arrow() for c in b.columns])

    want, seen, kept = expected_rows(jt, with_filter, shape)
    problems = []
    if shape in ("chunked", "whole"):              # conditions on the inputs: every case emits rows, the filter removes some key-matched pairs and keeps some
        if not want:
            problems.append("the oracle emits no row: the inputs do not exercise this case")
        if with_filter and not 0 < kept < seen:
            problems.append(f"the filter kept {kept} of {seen} key-matched pairs: it must remove some and keep some")
    if sort_rows(got) != sort_rows(want):
        problems.append(f"rows differ from the oracle's as a multiset ({len(got)} rows, the oracle has {len(want)})")
    elif jt in ("Inner", "RightSemi", "RightAnti") and got != want:
        problems.append("the rows are the oracle's, their order is not")
    return problems


@pytest.mark.gpu
def test_hash_join_with_filter_all_types_both_routes(ctx):
    """All 8 join types x (no filter, left.v > right.w) x 4 shapes = 64 cases under one test id, every one checked and every failing one named.
    Multiset of rows equals the oracle's for every case; exact order for the probe-order preserving types.  A NULL w gives a NULL filter result,
    which drops the pair."""
    failed = {}
    for shape in SHAPES:
        for with_filter in (False, True):
            for jt in JOIN_TYPES:
                problems = case_problems(ctx, jt, with_filter, shape)
                if problems:
                    failed[f"{jt}-{'filter' if with_filter else 'nofilter'}-{shape}"] = problems
    assert not failed, "\n".join(f"{case}: {'; '.join(msgs)}" for case, msgs in failed.items())


def test_join_filter_with_null_index_arrays_is_refused():
    """A JoinFilter that names columns (nf > 0) without the (side, index) arrays is InvalidArgument for all three join constructors."""
    from dfgpu import capi
    lib = capi.load_library()
    INVALID_ARGUMENT = 5
    handles = []

    def made(call):
        out = C.c_void_p(); assert call(C.byref(out)) == 0; handles.append(out); return out

    sizes = (C.c_int32 * 1)(0); none = (C.c_void_p * 1)()
    left = made(lambda o: lib.dfgpu_plan_memory(none, sizes, 1, o)); right = made(lambda o: lib.dfgpu_plan_memory(none, sizes, 1, o))
    col = made(lambda o: lib.dfgpu_expr_column(b"x", 0, o))
    on = (C.c_void_p * 1)(col.value)
    try:
        for side_idx in ((None, None), ((C.c_int32 * 1)(0), None), (None, (C.c_int32 * 1)(0))):
            fs, fi = side_idx
            out = C.c_void_p()
            assert lib.dfgpu_plan_hash_join(left, right, on, on, 1, col, fs, fi, 1, capi.JOIN_INNER, 0, 0, C.byref(out)) == INVALID_ARGUMENT
            assert lib.dfgpu_plan_sort_merge_join(left, right, on, on, 1, col, fs, fi, 1, capi.JOIN_INNER, 0, C.byref(out)) == INVALID_ARGUMENT
            assert lib.dfgpu_plan_nested_loop_join(left, right, col, fs, fi, 1, capi.JOIN_INNER, C.byref(out)) == INVALID_ARGUMENT
            assert not out.value
    finally:
        lib.dfgpu_expr_free(handles[2]); lib.dfgpu_plan_free(handles[1]); lib.dfgpu_plan_free(handles[0])
