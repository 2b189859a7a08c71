"""-m gpu: every column kernel on array views (tests/views.py) -- windows into a larger parent array, as dfgpu_array_slice hands them out and as
collect, the partition outputs, the sort-merge join chunks, the spill runs, TopK and limit pass them on.

Every case makes two assertions, both bit for bit: the result over the view equals the plain reference for the window (the C oracle, pyarrow, or
numpy's stable lexsort -- whichever the operator's own test file uses), and it equals the result of the same call on a freshly imported copy of the
window.  Every view-class case also asserts, from Array.describe(), that the slice really is a view; the control arm (class E) that it is a copy.
A Boolean or nullable result has its null_count and dfgpu_mask_count checked and is passed on into filter / mask_to_indices, which proves that
whatever its last word holds past `length` is harmless.

What runs where (view classes of tests/views.py; "all kinds" = test_gpu_core.KINDS):
  hash_columns               A-E, view of a view, zero length, whole parent: all kinds; one 8-byte column at rows 1 / 3 / 65 (k_hash_rows, asserted from the profile); 7 mixed columns
  take                       values, indices (UInt32 A, nullable UInt64 C) and both as views: all kinds
  filter, mask_to_indices    values, mask (C) and both as views: all kinds
  binary                     every opcode; view left / right / both at different rows / against a scalar; A and C over Int16, Int32 (/ %), Int64, Float64, Decimal128, Utf8, Boolean;
                             dictionary against a literal (D): the eight comparisons, the opcodes dfgpu_binary takes for that shape.  Arithmetic on Utf8 / Boolean and AND / OR on numbers are type errors in the oracle too, hence not cases.
  not, is_null, negative, in_list, cast (CASTS)      A, C, E, view of a view, zero length
  sort_to_indices(_keys)     keys A + C + Utf8 B at different rows; one-block, fused small passes, word mode + one sweep (2^20 + 4321 rows), each asserted from the profile
  hash_partition, partition_columns     keys A + C, payload 8 / 4 / 16 bytes + Utf8 B + nullable C, mask C; 3 and 64 partitions
  JoinTable                  keys A (dense and sparse Int64), C (nullable Int32), Utf8 B, Int64 A + Utf8 B, Int64 A + nullable Int32 C (also null_equals_null); build and probe masks C
  radix-partitioned join     keys A (Int64 over the whole range), C (the same, nullable), Utf8 B and Int64 A + Utf8 B (hashed keys, pj_verify asserted); build and probe masks C
  update_batch, update_batch_multi, merge_batch      values A / C, group ids A, opt_filter C.  Float64 SUM / AVG run over multiples of 1/4 so that the order of the atomic additions cannot show
  update_batch_fused         Decimal128 views are taken at every row; Float64 views at an odd row answer NotImplemented (asserted), and the plan test shows AggregateExec's fallback
  GroupValues.intern         dictionary keys whose codes are views at an odd row: k_dense_first_fast behind the alignment guard (asserted from the profile), ids also as a deferred recipe
  concat                     A / B / E at an odd row, views of views, a zero-length view in the middle, C ragged, only NULLs; then slice, concat again, export
  plans                      MemoryExec over view batches at row 1, 64 (ragged) and 128 (ragged): Filter -> Projection -> Aggregate, fused aggregate, SortExec with fetch, HashJoinExec"""
import decimal
import zlib

import numpy as np
import pyarrow as pa
import pytest

import views
from oracle import pyoracle as po
from test_gpu_core import KINDS, rand_array
from test_gpu_expr import CASTS, CMP, OPCODE, same
from test_gpu_pjoin import forced
from views import VIEW_CASES, VIEW_CASES_SHORT, ViewCase, assert_view, plain

pytestmark = pytest.mark.gpu
BOOL = 1


def ids(cases):
    return [c.id for c in cases]


def rng_for(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def same_arrow(a, b):
    return same(plain(a), plain(b))


def check_mask(ctx, got, want):
    """a Boolean result: dfgpu_mask_count, then the result as the mask of mask_to_indices and filter"""
    truth = np.asarray(want.fill_null(False), dtype=bool)
    assert ctx.mask_count(got) == int(truth.sum())
    assert np.array_equal(ctx.mask_to_indices(got).to_numpy(), np.flatnonzero(truth).astype(np.uint32))
    rows = ctx.from_arrow(pa.array(np.arange(len(want), dtype=np.int64)))
    assert np.array_equal(ctx.filter(rows, got).to_numpy(), np.flatnonzero(truth))


def check(ctx, got, fresh, want, what=""):
    """device result over views `got`, over fresh arrays `fresh`, reference `want`"""
    ga = got.to_arrow()
    assert same_arrow(ga, want), what
    assert same_arrow(ga, fresh.to_arrow()), what
    assert got.null_count == want.null_count, what
    if got.type == BOOL:
        check_mask(ctx, got, want)


def misaligned(a):
    return (a.describe().values or 0) & 15 != 0


# ------------------------------------------------------------------ hash_columns
@pytest.mark.parametrize("case", VIEW_CASES, ids=ids(VIEW_CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_hash_columns_of_one_view(ctx, kind, case):
    v, exp = case.make(ctx, kind, rng_for("hash", kind, case.id))
    got = ctx.hash_columns([v]).to_numpy()
    assert np.array_equal(got, po.create_hashes([exp]))
    assert np.array_equal(got, ctx.hash_columns([ctx.from_arrow(exp)]).to_numpy())


def profiled(ctx, fn):
    """-> (fn(), names of the kernels that ran inside it)"""
    ctx.profile_select(None); ctx.profile_enable(True); ctx.profile_read()
    try:
        out = fn()
        ks = set(ctx.profile_read())
    finally:
        ctx.profile_enable(False)
    return out, ks


@pytest.mark.parametrize("off", [1, 3, 65, 64])
@pytest.mark.parametrize("kind", ["int64", "uint64", "float64"])
def test_hash_of_one_8_byte_view_at_an_odd_row_takes_the_row_kernel(ctx, kind, off):
    """k_hash_i64 loads two keys at once and is gated on a 16-byte aligned pointer (hash_keys_device): a single non-null 8-byte column at an odd row
    is 8 but not 16 bytes aligned and goes through k_hash_rows; the profile shows which of the two ran.  Row 64 is the aligned arm."""
    for n in (1, 2, 4097):
        exp = rand_array(kind, n, 0.0, rng_for("hash8", kind, off, n))
        v, _ = views.as_view(ctx, exp, off)
        assert_view(v)
        assert not misaligned(v.parent) and misaligned(v) == (off % 2 == 1)
        h, ks = profiled(ctx, lambda: ctx.hash_columns([v]))
        assert ("k_hash_rows" in ks) == (off % 2 == 1) and ("k_hash_i64" in ks) == (off % 2 == 0), ks
        got = h.to_numpy()
        assert np.array_equal(got, po.create_hashes([exp]))
        assert np.array_equal(got, ctx.hash_columns([ctx.from_arrow(exp)]).to_numpy())


def test_hash_of_seven_columns_of_mixed_view_classes(ctx):
    rng = rng_for("hash7")
    spec = [("int64", ViewCase("A", 1, 961)), ("utf8", ViewCase("B", 3, 961)), ("decimal", ViewCase("C", 64, 961, "some")), ("dict", ViewCase("D", 65, 961)),
            ("float64", ViewCase("C", 128, 961, "clean")), ("bool", ViewCase("C", 64, 961)), ("date32", ViewCase("E", 1, 961, "some"))]
    made = [c.make(ctx, k, rng) for k, c in spec]
    got = ctx.hash_columns([v for v, _ in made]).to_numpy()
    assert np.array_equal(got, po.create_hashes([e for _, e in made]))
    assert np.array_equal(got, ctx.hash_columns([ctx.from_arrow(e) for _, e in made]).to_numpy())


# ------------------------------------------------------------------ take / filter / mask_to_indices
@pytest.mark.parametrize("case", VIEW_CASES_SHORT, ids=ids(VIEW_CASES_SHORT))
@pytest.mark.parametrize("kind", KINDS)
def test_take_with_values_and_indices_as_views(ctx, kind, case):
    """values as a view, indices as a view (UInt32 class A at row 3, nullable UInt64 class C at row 64), both; the rows around an index window hold
    indices far outside the values, so an index read from outside the window is an error"""
    rng = rng_for("take", kind, case.id)
    v, exp = case.make(ctx, kind, rng)
    n, m = case.n, (1217 if case.n else 0)
    idx = rng.integers(0, max(n, 1), m)
    i32 = pa.array(idx.astype(np.uint32)); i64 = pa.array(idx.astype(np.uint64), mask=rng.random(m) < 0.1)
    iv32, _ = ViewCase("i32", 3, m).make(ctx, "uint32", rng, arr=i32)
    iv64, _ = ViewCase("i64", 64, m, "some").make(ctx, "uint64", rng, arr=i64)
    fresh = ctx.from_arrow(exp)
    for ia, iv in ((i32, iv32), (i64, iv64)):
        want = plain(exp).take(ia)
        oidx = np.where(np.asarray(ia.is_null()), -1, idx)
        assert same_arrow(want, po.take(exp, oidx))
        base = ctx.take(fresh, ctx.from_arrow(ia))
        for vals, ind in ((v, ctx.from_arrow(ia)), (fresh, iv), (v, iv)):
            got = ctx.take(vals, ind)
            assert same_arrow(got.to_arrow(), want) and same_arrow(got.to_arrow(), base.to_arrow())
            assert got.null_count == want.null_count


@pytest.mark.parametrize("case", VIEW_CASES_SHORT, ids=ids(VIEW_CASES_SHORT))
@pytest.mark.parametrize("kind", KINDS)
def test_filter_and_mask_to_indices_with_values_and_mask_as_views(ctx, kind, case):
    rng = rng_for("filter", kind, case.id)
    v, exp = case.make(ctx, kind, rng)
    m = rand_array("bool", case.n, 0.15, rng)
    mv, _ = ViewCase("mask", 128, case.n, "some").make(ctx, "bool", rng, arr=m)           # class C: values and validity words shared with the parent
    want = plain(exp).filter(m, null_selection_behavior="drop")
    assert same_arrow(want, po.filter_(exp, m))
    fresh, mfresh = ctx.from_arrow(exp), ctx.from_arrow(m)
    base = ctx.filter(fresh, mfresh)
    for vals, mask in ((v, mfresh), (fresh, mv), (v, mv)):
        got = ctx.filter(vals, mask)
        assert same_arrow(got.to_arrow(), want) and same_arrow(got.to_arrow(), base.to_arrow())
        assert got.null_count == want.null_count
    assert mv.null_count == m.null_count
    check_mask(ctx, mv, m)


# ------------------------------------------------------------------ expressions
BIN_CASES = [ViewCase("A", 3, 1000), ViewCase("C", 64, 961, "some")]
BIN_RIGHT = {"A": ViewCase("A-right", 65, 1000), "C": ViewCase("C-right", 128, 961, "some")}
ARITH = {"int16": ["+", "-", "*"], "int32": ["/", "%"], "int64": ["+", "-", "*", "/", "%"], "float64": ["+", "-", "*", "/", "%"], "decimal": ["+", "-", "*", "/", "%"],
         "utf8": [], "bool": ["AND", "OR"]}
BINARY = [(op, kind) for kind, ops in ARITH.items() for op in ops + (CMP if kind != "int32" else [])]
assert {op for op, _ in BINARY} == set(OPCODE)          # arithmetic on Utf8 / Boolean and Kleene logic on numbers are type errors in the oracle as well: not operators


def nonzero(a):
    one = decimal.Decimal(1) if pa.types.is_decimal(a.type) else 1
    return pa.array([None if x is None else (x if x != 0 else one) for x in a.to_pylist()], type=a.type)


@pytest.mark.parametrize("op,kind", BINARY, ids=[f"{k}-{o.replace(' ', '_')}" for o, k in BINARY])
def test_binary_with_views_on_either_side(ctx, op, kind):
    """a view on the left, on the right, on both sides at different row offsets, and a view against a scalar; the rows around the windows hold the types'
    extremes, so a row evaluated outside the window overflows or divides where the window does not"""
    for case in BIN_CASES:
        rng = rng_for("binary", op, kind, case.id)
        l, r = case.window(kind, rng), case.window(kind, rng)
        if kind in ("int16", "int64", "float64", "decimal") and op in CMP:
            r = pa.array([lv if i % 3 == 0 else rv for i, (lv, rv) in enumerate(zip(l.to_pylist(), r.to_pylist()))], type=r.type)
        if op in ("/", "%") and kind != "float64":
            r = nonzero(r)
        lv, _ = case.make(ctx, kind, rng, arr=l)
        rv, _ = BIN_RIGHT[case.id].make(ctx, kind, rng, arr=r)
        lf, rf = ctx.from_arrow(l), ctx.from_arrow(r)
        want = po.binary(op, l, r)
        base = ctx.binary(OPCODE[op], lf, rf)
        for a, b in ((lv, rf), (lf, rv), (lv, rv)):
            check(ctx, ctx.binary(OPCODE[op], a, b), base, want, (op, kind, case.id))
        s = r.drop_null().slice(0, 1)
        sf = ctx.from_arrow(s)
        check(ctx, ctx.binary(OPCODE[op], lv, sf, False, True), ctx.binary(OPCODE[op], lf, sf, False, True), po.binary(op, l, s, r_scalar=True), (op, kind, case.id, "scalar"))
        check(ctx, ctx.binary(OPCODE[op], sf, rv, True, False), ctx.binary(OPCODE[op], sf, rf, True, False), po.binary(op, s, r, l_scalar=True), (op, kind, case.id, "scalar-left"))


@pytest.mark.parametrize("case", VIEW_CASES_SHORT, ids=ids(VIEW_CASES_SHORT))
@pytest.mark.parametrize("op", CMP, ids=[o.replace(" ", "_") for o in CMP])
def test_dictionary_view_against_a_literal(ctx, op, case):
    """class D: the codes are a view (A or C), the dictionary is the parent's and holds entries no code of the window points at"""
    rng = rng_for("dictlit", op, case.id)
    col = case.window("dict", rng)
    v, _ = case.make(ctx, "dict", rng, arr=col)
    lit = pa.array(["BUILDING0"], type=pa.utf8()); dl = ctx.from_arrow(lit)
    p = col.cast(pa.utf8())
    check(ctx, ctx.binary(OPCODE[op], v, dl, False, True), ctx.binary(OPCODE[op], ctx.from_arrow(col), dl, False, True), po.binary(op, p, lit, r_scalar=True))
    check(ctx, ctx.binary(OPCODE[op], dl, v, True, False), ctx.binary(OPCODE[op], dl, ctx.from_arrow(col), True, False), po.binary(op, lit, p, l_scalar=True))


@pytest.mark.parametrize("case", VIEW_CASES_SHORT, ids=ids(VIEW_CASES_SHORT))
def test_not_is_null_negative_in_list_on_views(ctx, case):
    rng = rng_for("unary", case.id)
    v, b = case.make(ctx, "bool", rng)
    check(ctx, ctx.not_(v), ctx.not_(ctx.from_arrow(b)), po.not_(b))
    for kind in ["int64", "utf8", "dict", "decimal", "bool", "int8"]:
        v, a = case.make(ctx, kind, rng)
        for neg in (False, True):
            check(ctx, ctx.is_null(v, neg), ctx.is_null(ctx.from_arrow(a), neg), po.is_null(a, neg), (kind, neg))
    for kind in ["int32", "int64", "float64", "decimal"]:
        # the windows stay clear of the type's minimum; the rows around them hold it (views.pad_rows)
        v, a = case.make(ctx, kind, rng)
        check(ctx, ctx.negative(v), ctx.negative(ctx.from_arrow(a)), po.negative(a), kind)
    a = pa.array(rng.integers(0, 20, case.n), mask=(rng.random(case.n) < 0.1) if case.nullable and case.nulls != "clean" else None)
    if case.nulls == "all":
        a = pa.nulls(case.n, pa.int64())
    v, _ = case.make(ctx, "int64", rng, arr=a)
    for lst in [pa.array([1, 5, 7]), pa.array([1, None, 7]), pa.array([], type=pa.int64())]:
        for neg in (False, True):
            check(ctx, ctx.in_list(v, ctx.from_arrow(lst), neg), ctx.in_list(ctx.from_arrow(a), ctx.from_arrow(lst), neg), po.in_list(a, lst, neg))
    v, u = case.make(ctx, "utf8", rng)
    lst = pa.array(["BUILDING0", "ASIA3", "a1"])
    check(ctx, ctx.in_list(v, ctx.from_arrow(lst)), ctx.in_list(ctx.from_arrow(u), ctx.from_arrow(lst)), po.in_list(u, lst))


@pytest.mark.parametrize("case", VIEW_CASES_SHORT, ids=ids(VIEW_CASES_SHORT))
@pytest.mark.parametrize("kind,to", [c for c in CASTS if c[1] is not None], ids=[f"{k}-to-{t}" for k, t in CASTS if t is not None])
def test_cast_of_a_view(ctx, kind, to, case):
    import dfgpu
    v, a = case.make(ctx, kind, rng_for("cast", kind, str(to), case.id))
    code = {pa.int32(): 4, pa.int64(): 5, pa.float32(): 10, pa.float64(): 11, pa.date32(): 12}.get(to)
    args = (dfgpu.capi.DECIMAL128, to.precision, to.scale) if pa.types.is_decimal(to) else (code,)
    check(ctx, ctx.cast(v, *args), ctx.cast(ctx.from_arrow(a), *args), po.cast(a, to))


# ------------------------------------------------------------------ sort
def sort_paths(ctx, cols, desc, nf, fetch=None, keys=False):
    ctx.profile_select(None); ctx.profile_enable(True); ctx.profile_read()
    try:
        out = ctx.sort_to_indices_keys(cols, desc, nf, fetch) if keys else (ctx.sort_to_indices(cols, desc, nf, fetch), None)
        ks = set(ctx.profile_read())
    finally:
        ctx.profile_enable(False)
    return out[0], out[1], ks


@pytest.mark.parametrize("n,path", [(0, None), (1, None), (8192, "radix_pass_one_block"), (70001, "radix_pass")])
def test_sort_keys_as_views_one_block_and_fused_small_passes(ctx, n, path):
    """two fixed-width key columns at different row offsets (nullable class C at row 64 / 128, non-null class A at row 3) and a Utf8 class B tie-break key
    at row 1; the profile shows which pass kernels ran"""
    rng = rng_for("sort", n)
    a = pa.array(rng.integers(0, 40, n).astype(np.int32), mask=rng.random(n) < 0.1)
    b = pa.array(rng.integers(-5, 5, n).astype(np.int64))
    u = pa.array(np.array(["", "a", "ab", "b", "zz", "abc", "日本"], dtype=object)[rng.integers(0, 7, n)], type=pa.utf8())
    for off_a in (64, 128):
        va, _ = ViewCase("C", off_a, n, "some").make(ctx, "int32", rng, arr=a)
        vb, _ = ViewCase("A", 3, n).make(ctx, "int64", rng, arr=b)
        vu, _ = ViewCase("B", 1, n).make(ctx, "utf8", rng, arr=u)
        for cols, fresh, host in (([va, vb], [a, b], [a, b]), ([va, vu, vb], [a, u, b], [a, u, b])):
            desc, nf = [True, False, True][:len(cols)], [False, True, True][:len(cols)]
            want = po.lexsort_to_indices(host, desc, nf)
            for fetch in (None, n // 3):
                got, sk, ks = sort_paths(ctx, cols, desc, nf, fetch, keys=True)
                for c, k in zip(host, sk):          # a key column the sort rebuilt as a by-product equals take(column, indices)
                    assert k is None or k.to_arrow().equals(c.take(pa.array(want if fetch is None else want[:fetch])))
                base = ctx.sort_to_indices([ctx.from_arrow(c) for c in fresh], desc, nf, fetch).to_numpy()
                w = want if fetch is None else want[:fetch]
                assert np.array_equal(got.to_numpy(), w) and np.array_equal(got.to_numpy(), base)
                if path and fetch is None:
                    assert path in ks, ks
    # numpy's stable lexsort over the two integer keys: NULLs last in the descending first key, second key ascending
    if n:
        ka = np.where(np.asarray(a.is_null()), np.int64(1 << 40), -np.asarray(a.fill_null(0)).astype(np.int64))
        got = ctx.sort_to_indices([va, vb], [True, False], [False, True]).to_numpy()
        assert np.array_equal(got.astype(np.int64), np.lexsort((np.arange(n), np.asarray(b), ka)))


@pytest.mark.parametrize("fetch", [None, 700_000])
def test_sort_keys_as_views_word_mode_and_one_sweep(ctx, fetch):
    """2^20 + 4321 rows: the packed keys and the row number share one word, the passes are the one-sweep ones; every rebuilt key column equals take(column, indices)"""
    rng = rng_for("sort-large")
    n = (1 << 20) + 4321
    cols = [pa.array(rng.integers(-100, 100, n).astype(np.int16)), pa.array(rng.integers(0, 1000, n), mask=rng.random(n) < 0.1), pa.array(rng.integers(-2**10, 2**10, n).astype(np.int64))]
    desc, nf = [False, True, True], [True, False, True]
    vs = [ViewCase("A", 1, n).make(ctx, "int16", rng, arr=cols[0])[0], ViewCase("C", 64, n, "some").make(ctx, "int64", rng, arr=cols[1])[0],
          ViewCase("A", 3, n).make(ctx, "int64", rng, arr=cols[2])[0]]
    assert misaligned(vs[0]) and misaligned(vs[2])
    idx, sk, ks = sort_paths(ctx, vs, desc, nf, fetch, keys=True)
    assert "sort_key_encode" in ks and (fetch is not None or "sort_pass_onesweep" in ks), ks
    want = po.lexsort_to_indices(cols, desc, nf)
    want = want if fetch is None else want[:fetch]
    bidx, bsk = ctx.sort_to_indices_keys([ctx.from_arrow(c) for c in cols], desc, nf, fetch)
    assert np.array_equal(idx.to_numpy(), want) and np.array_equal(idx.to_numpy(), bidx.to_numpy())
    assert [k is not None for k in sk] == [True, False, True] == [k is not None for k in bsk]
    for c, k in zip(cols, sk):
        if k is not None:
            assert k.to_arrow().equals(c.take(pa.array(want)))
    assert np.array_equal(ctx.sort_to_indices(vs, desc, nf, fetch).to_numpy(), want)


# ------------------------------------------------------------------ hash_partition / partition_columns
@pytest.mark.parametrize("nparts", [3, 64])
@pytest.mark.parametrize("offs", [(1, 3, 128), (65, 64, 64)], ids=["odd-rows", "row-65-and-64"])
@pytest.mark.parametrize("n", [0, 1, 4097, 50001])
def test_partition_with_keys_payload_and_mask_as_views(ctx, nparts, offs, n):
    """keys (Int64 class A, nullable Int32 class C), payload columns of 8, 4 and 16 bytes, Utf8 (class B) and a nullable one (class C), and the selection mask
    (class C) are all views; rows go to hash % n in input order and the columns written in the same pass equal take(column, indices)"""
    rng = rng_for("partition", nparts, offs, n)
    oa, ob, oc = offs
    keys = [pa.array(rng.integers(0, 5000, n).astype(np.int64)), pa.array(rng.integers(-2500, 2500, n).astype(np.int32), mask=rng.random(n) < 0.1)]
    cols = [pa.array(rng.integers(-2**60, 2**60, n)), pa.array(rng.integers(0, 100, n).astype(np.int32)),
            pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in rng.integers(-10**12, 10**12, n)], type=pa.decimal128(15, 2)),
            pa.array([f"s{i % 13}" for i in range(n)], type=pa.utf8()), pa.array(rng.integers(0, 1000, n), mask=rng.random(n) < 0.2)]
    kv = [ViewCase("A", oa, n).make(ctx, "int64", rng, arr=keys[0])[0], ViewCase("C", oc, n, "some").make(ctx, "int32", rng, arr=keys[1])[0]]
    cv = [ViewCase("A", o, n).make(ctx, k, rng, arr=c)[0] for o, k, c in zip((oa, ob, oa, ob), ("int64", "int32", "decimal", "utf8"), cols[:4])]
    cv.append(ViewCase("C", oc, n, "some").make(ctx, "int64", rng, arr=cols[4])[0])
    kf, cf = [ctx.from_arrow(k) for k in keys], [ctx.from_arrow(c) for c in cols]
    # hash_partition: indices and counts
    oidx, ocounts = po.hash_partition(keys, nparts)
    idx, counts = ctx.hash_partition(kv, nparts)
    bidx, bcounts = ctx.hash_partition(kf, nparts)
    assert counts == ocounts.tolist() == bcounts and np.array_equal(idx.to_numpy(), oidx) and np.array_equal(idx.to_numpy(), bidx.to_numpy())
    # partition_columns, without and with a selection
    mask = rng.random(n) < 0.4
    mv, _ = ViewCase("C", oc, n).make(ctx, "bool", rng, arr=pa.array(mask))
    for m_host, m_view, m_fresh in ((None, None, None), (mask, mv, ctx.from_arrow(pa.array(mask)))):
        sel = np.arange(n) if m_host is None else np.flatnonzero(m_host)
        oidx, ocounts = po.hash_partition([k.take(pa.array(sel)) for k in keys], nparts)
        rows = sel[oidx] if n else oidx
        outs, idx, counts = ctx.partition_columns(kv, nparts, cv, mask=m_view)
        bouts, bidx, bcounts = ctx.partition_columns(kf, nparts, cf, mask=m_fresh)
        assert counts == ocounts.tolist() == bcounts and sum(counts) == len(sel)
        assert np.array_equal(idx.to_numpy(), rows) and np.array_equal(idx.to_numpy(), bidx.to_numpy())
        # fixed-width without validity: written in the same pass; Utf8 and the column with a validity buffer go through the indices (a fresh column of 0 or 1 rows has no
        # NULL, hence no validity buffer, and is written directly -- the view keeps its parent's)
        assert [o is not None for o in outs] == [True, True, True, False, False] and [o is not None for o in bouts[:4]] == [True, True, True, False]
        for c, o in enumerate(outs):
            if o is not None:
                assert o.to_arrow().equals(cols[c].take(pa.array(rows))) and o.to_arrow().equals(bouts[c].to_arrow())


# ------------------------------------------------------------------ joins
def join_pairs(ctx, bcols, pcols, bmask, pmask):
    import dfgpu
    table = dfgpu.JoinTable(ctx, bcols, mask=bmask)
    bi, pi = table.probe(pcols, mask=pmask)
    return bi.to_numpy().astype(np.int64), pi.to_numpy().astype(np.int64)


def join_inputs(shape, rng):
    """-> (build key columns, probe key columns, [(kind, nulls) per key column])"""
    nb, npr = 6001, 40001
    words = np.array([f"k{i:05d}" + "x" * (i % 5) for i in range(nb)], dtype=object)[rng.permutation(nb)]
    pick = rng.integers(0, nb, npr)
    if shape == "int64-class-A":
        return [pa.array(rng.permutation(np.arange(nb, dtype=np.int64) * 7 - 9000))], [pa.array(rng.integers(-10000, 7 * nb, npr).astype(np.int64))], [("int64", "none")]
    if shape == "int64-dense-class-A":          # strictly increasing dense keys: the rank index and the bitmap probe, which reads two keys per load
        return [pa.array(np.arange(nb, dtype=np.int64) * 3 + 5)], [pa.array(rng.integers(0, 3 * nb + 10, npr).astype(np.int64))], [("int64", "none")]
    if shape in ("int64-wide-class-A", "int64-wide-nullable-class-C"):          # unique keys spread over the whole Int64 range: no dense domain, the radix-partitioned join takes them
        k = np.unique(rng.integers(-(1 << 62), 1 << 62, nb + 64))[:nb]; rng.shuffle(k)
        pk = np.where(rng.random(npr) < 0.3, k[pick], rng.integers(-(1 << 62), 1 << 62, npr))
        nulls = shape.endswith("C")
        return [pa.array(k, mask=(rng.random(nb) < 0.1) if nulls else None)], [pa.array(pk, mask=(rng.random(npr) < 0.1) if nulls else None)], [("int64", "some" if nulls else "none")]
    if shape == "int32-nullable-class-C":
        return ([pa.array(rng.integers(0, 20000, nb).astype(np.int32), mask=rng.random(nb) < 0.1)], [pa.array(rng.integers(0, 20000, npr).astype(np.int32), mask=rng.random(npr) < 0.1)],
                [("int32", "some")])
    pw = pa.array(np.where(rng.random(npr) < 0.4, words[pick], np.array([f"q{i}" for i in range(npr)], dtype=object)), type=pa.utf8())
    if shape == "utf8-class-B":
        return [pa.array(words, type=pa.utf8())], [pw], [("utf8", "none")]
    assert shape == "int64-A-and-utf8-B"          # some probe rows match in the second column only
    k0 = rng.integers(0, 50, nb)
    return [pa.array(k0), pa.array(words, type=pa.utf8())], [pa.array(np.where(rng.random(npr) < 0.7, k0[pick], -1)), pw], [("int64", "none"), ("utf8", "none")]


def check_join_over_views(ctx, shape, masked, offs):
    """offs = (row of the build windows, row of the probe windows); a second key column sits two rows (class A / B) further on"""
    rng = rng_for("join", shape, masked, offs)
    b, p, cols = join_inputs(shape, rng)
    ob, op_ = offs
    bv = [ViewCase("b", ob + 2 * c, len(a), nulls).make(ctx, kind, rng, arr=a)[0] for c, (a, (kind, nulls)) in enumerate(zip(b, cols))]
    pv = [ViewCase("p", op_ + 2 * c, len(a), nulls).make(ctx, kind, rng, arr=a)[0] for c, (a, (kind, nulls)) in enumerate(zip(p, cols))]
    nb, npr = len(b[0]), len(p[0])
    bm = pm = bmv = pmv = bmf = pmf = None
    if masked:
        bm, pm = rng.random(nb) < 0.8, rng.random(npr) < 0.6
        bmv, _ = ViewCase("bm", 64, nb).make(ctx, "bool", rng, arr=pa.array(bm))
        pmv, _ = ViewCase("pm", 128, npr).make(ctx, "bool", rng, arr=pa.array(pm))
        bmf, pmf = ctx.from_arrow(pa.array(bm)), ctx.from_arrow(pa.array(pm))
    bsel = np.arange(nb) if bm is None else np.flatnonzero(bm)
    psel = np.arange(npr) if pm is None else np.flatnonzero(pm)
    want = po.hash_join([[c.take(pa.array(bsel)) for c in b]], [[c.take(pa.array(psel)) for c in p]], "Inner", False, batch_size=1 << 40)
    assert len(want.probe_idx) > 100
    bi, pi = join_pairs(ctx, bv, pv, bmv, pmv)
    fbi, fpi = join_pairs(ctx, [ctx.from_arrow(c) for c in b], [ctx.from_arrow(c) for c in p], bmf, pmf)
    assert np.array_equal(bi, bsel[want.build_idx]) and np.array_equal(pi, psel[want.probe_idx])
    assert np.array_equal(bi, fbi) and np.array_equal(pi, fpi)


# columns without a bitmap are views at every row; nullable ones at multiples of 64 only (elsewhere dfgpu_array_slice copies: class E)
OFFS_ANY = [(1, 3), (65, 1), (64, 128)]
OFFS_64 = [(64, 128), (128, 64)]
JOIN_CASES = [(s, o) for s in ("int64-class-A", "int64-dense-class-A", "utf8-class-B", "int64-A-and-utf8-B") for o in OFFS_ANY] + [("int32-nullable-class-C", o) for o in OFFS_64]
RADIX_CASES = [(s, o) for s in ("int64-wide-class-A", "utf8-class-B", "int64-A-and-utf8-B") for o in OFFS_ANY[::2]] + [("int64-wide-nullable-class-C", o) for o in OFFS_64]
join_ids = lambda cases: [f"{s}-rows-{o[0]}-{o[1]}" for s, o in cases]


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask-views"])
@pytest.mark.parametrize("shape,offs", JOIN_CASES, ids=join_ids(JOIN_CASES))
def test_join_table_over_view_keys_and_view_masks(ctx, shape, offs, masked):
    check_join_over_views(ctx, shape, masked, offs)


@pytest.mark.parametrize("null_equals_null", [False, True])
def test_join_table_over_two_view_key_columns(ctx, null_equals_null):
    """(Int64 class A at an odd row, nullable Int32 class C) on both sides, at different rows"""
    import dfgpu
    rng = rng_for("join2", null_equals_null)
    nb, npr = 5003, 30011
    mk = lambda n: [pa.array(rng.integers(0, 300, n).astype(np.int64)), pa.array(rng.integers(0, 40, n).astype(np.int32), mask=rng.random(n) < 0.1)]
    b, p = mk(nb), mk(npr)
    bv = [ViewCase("b0", 1, nb).make(ctx, "int64", rng, arr=b[0])[0], ViewCase("b1", 64, nb, "some").make(ctx, "int32", rng, arr=b[1])[0]]
    pv = [ViewCase("p0", 3, npr).make(ctx, "int64", rng, arr=p[0])[0], ViewCase("p1", 128, npr, "some").make(ctx, "int32", rng, arr=p[1])[0]]
    want = po.hash_join([b], [p], "Inner", null_equals_null, batch_size=1 << 40)
    bi, pi = dfgpu.JoinTable(ctx, bv, null_equals_null=null_equals_null).probe(pv)
    fbi, fpi = dfgpu.JoinTable(ctx, [ctx.from_arrow(c) for c in b], null_equals_null=null_equals_null).probe([ctx.from_arrow(c) for c in p])
    assert len(want.probe_idx) > 100
    assert np.array_equal(bi.to_numpy().astype(np.int64), want.build_idx) and np.array_equal(pi.to_numpy().astype(np.int64), want.probe_idx)
    assert np.array_equal(bi.to_numpy(), fbi.to_numpy()) and np.array_equal(pi.to_numpy(), fpi.to_numpy())


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask-views"])
@pytest.mark.parametrize("shape,offs", RADIX_CASES, ids=join_ids(RADIX_CASES))
def test_radix_partitioned_join_over_view_keys_and_view_masks(ctx, shape, offs, masked):
    """the same shapes through the radix-partitioned join: integer keys travel as they are, Utf8 keys (alone, and behind an Int64 column) as 64-bit key hashes whose pairs
    are verified in the columns -- the pass that reads offsets[] against the values base of the view"""
    with forced(ctx, 640) as f:
        check_join_over_views(ctx, shape, masked, offs)
        ran = f.kernels()
    assert "pj_join" in ran, ran
    if "utf8" in shape:
        assert "pj_verify" in ran, ran


# ------------------------------------------------------------------ accumulators
KIND = {"SUM": 0, "AVG": 1, "COUNT": 2, "MIN": 3, "MAX": 4}
# exact results only: Float64 SUM / AVG add in an order the atomics choose, so they appear with values whose sums are exact (multiples of 1/4 of moderate size)
ACC_CASES = [("SUM", "int64"), ("SUM", "decimal"), ("AVG", "decimal"), ("COUNT", "utf8"), ("MIN", "float64"), ("MAX", "int16"), ("MIN", "decimal"), ("SUM", "quarters"), ("AVG", "quarters")]


def acc_values(kind, n, nulls, rng):
    if kind == "quarters":
        return pa.array(rng.integers(-4000, 4000, n) * 0.25, mask=(rng.random(n) < 0.2) if nulls else None)
    if kind == "int64":
        return pa.array(rng.integers(-2**40, 2**40, n), mask=(rng.random(n) < 0.2) if nulls else None)
    return rand_array(kind, n, 0.2 if nulls else 0.0, rng)


def new_acc(ctx, fun, arr):
    import dfgpu
    f = dfgpu.operators.field_of_array("v", ctx.from_arrow(arr.slice(0, 1)))
    return dfgpu.GroupsAccumulator(ctx, KIND[fun], f.dtype, f.precision, f.scale), po.Acc(fun, arr.type)


def assert_acc_equal(a, b, o):
    for x, y, z in zip(a.state(), b.state(), o.state()):
        assert same_arrow(x.to_arrow(), z) and same_arrow(x.to_arrow(), y.to_arrow())
    assert same_arrow(a.evaluate().to_arrow(), o.evaluate()) and same_arrow(a.evaluate().to_arrow(), b.evaluate().to_arrow())


@pytest.mark.parametrize("ngroups", [6, 300])
@pytest.mark.parametrize("cls", ["A-odd-rows", "C-row-64", "C-row-128-ragged"])
@pytest.mark.parametrize("fun,kind", ACC_CASES, ids=[f"{f}-{k}" for f, k in ACC_CASES])
def test_update_batch_with_values_group_ids_and_filter_as_views(ctx, fun, kind, cls, ngroups):
    """values (class A at an odd row, or class C), the UInt32 group ids (class A: rows 1 and 3 are 4 but not 16 bytes aligned) and opt_filter (class C) are views;
    the group ids around the window are far past total_num_groups, the filter bits around it are set"""
    rng = rng_for("acc", fun, kind, cls, ngroups)
    off, n, nulls = {"A-odd-rows": (1, 5000, False), "C-row-64": (64, 4096, True), "C-row-128-ragged": (128, 4033, True)}[cls]
    v = acc_values(kind, n, nulls, rng)
    g = rng.integers(0, ngroups, n)
    filt = pa.array(rng.random(n) < 0.7, mask=rng.random(n) < 0.05)
    vv, _ = ViewCase("v", off, n, "some" if nulls else "none").make(ctx, None, rng, arr=v)
    gv, _ = ViewCase("g", 3 if off == 1 else 1, n).make(ctx, "uint32", rng, arr=pa.array(g.astype(np.uint32)))
    fv, _ = ViewCase("f", 128, n, "some").make(ctx, "bool", rng, arr=filt)
    gf, ff = ctx.from_arrow(pa.array(g.astype(np.uint32))), ctx.from_arrow(filt)
    for use_filter in (False, True):
        a, o = new_acc(ctx, fun, v); b, _ = new_acc(ctx, fun, v)
        a.update_batch(vv, gv, fv if use_filter else None, ngroups)
        b.update_batch(ctx.from_arrow(v), gf, ff if use_filter else None, ngroups)
        o.update_batch(v, g, filt if use_filter else None, ngroups)
        assert_acc_equal(a, b, o)


@pytest.mark.parametrize("ngroups", [6, 9])
@pytest.mark.parametrize("cls", ["A-odd-rows", "C-row-64-ragged"])
def test_update_batch_multi_with_values_group_ids_and_filter_as_views(ctx, cls, ngroups):
    """Q1's accumulator list at once: up to 8 groups share passes, 9 take the single-accumulator paths"""
    import dfgpu
    rng = rng_for("acc-multi", cls, ngroups)
    off, n, nulls = {"A-odd-rows": (3, 30001, False), "C-row-64-ragged": (64, 30017, True)}[cls]
    g = rng.integers(0, ngroups, n)
    filt = pa.array(rng.random(n) < 0.8)
    cols = {"x": acc_values("quarters", n, nulls, rng), "y": acc_values("quarters", n, nulls, rng), "d": rand_array("decimal", n, 0.2 if nulls else 0.0, rng), "i": acc_values("int64", n, nulls, rng)}
    spec = [("SUM", "x"), ("AVG", "x"), ("SUM", "y"), ("AVG", "y"), ("COUNT", None), ("SUM", "d"), ("AVG", "d"), ("SUM", "i"), ("MIN", "x"), ("MAX", "d")]
    dv = {k: ViewCase(k, off, n, "some" if nulls else "none").make(ctx, None, rng, arr=c)[0] for k, c in cols.items()}
    df = {k: ctx.from_arrow(c) for k, c in cols.items()}
    gv, _ = ViewCase("g", 1, n).make(ctx, "uint32", rng, arr=pa.array(g.astype(np.uint32)))
    fv, _ = ViewCase("f", 64, n).make(ctx, "bool", rng, arr=filt)
    gf, ff = ctx.from_arrow(pa.array(g.astype(np.uint32))), ctx.from_arrow(filt)
    for use_filter in (False, True):
        accs, base, oaccs = [], [], []
        for fun, c in spec:
            if c is None:
                accs.append(dfgpu.GroupsAccumulator(ctx, KIND[fun], dfgpu.capi.INT64)); base.append(dfgpu.GroupsAccumulator(ctx, KIND[fun], dfgpu.capi.INT64)); oaccs.append(po.Acc(fun, pa.int64()))
            else:
                a, o = new_acc(ctx, fun, cols[c]); accs.append(a); oaccs.append(o); base.append(new_acc(ctx, fun, cols[c])[0])
        dfgpu.GroupsAccumulator.update_batch_multi(ctx, accs, [dv[c] if c else None for _, c in spec], [fv if use_filter else None] * len(spec), gv, ngroups)
        dfgpu.GroupsAccumulator.update_batch_multi(ctx, base, [df[c] if c else None for _, c in spec], [ff if use_filter else None] * len(spec), gf, ngroups)
        for (fun, c), a, b, o in zip(spec, accs, base, oaccs):
            o.update_batch(cols[c] if c else None, g, filt if use_filter else None, ngroups)
            assert_acc_equal(a, b, o)


@pytest.mark.parametrize("cls", ["A-odd-rows", "C-row-64-ragged"])
@pytest.mark.parametrize("fun,kind", [("SUM", "decimal"), ("AVG", "decimal"), ("AVG", "quarters"), ("MIN", "int64"), ("COUNT", "int64")])
def test_merge_batch_with_state_columns_as_views(ctx, fun, kind, cls):
    rng = rng_for("merge", fun, kind, cls)
    total = 4033 if cls != "A-odd-rows" else 5000
    v = acc_values(kind, 20000, True, rng)
    g = rng.integers(0, total, 20000)
    part, opart = new_acc(ctx, fun, v)
    part.update_batch(ctx.from_arrow(v), ctx.from_arrow(pa.array(g.astype(np.uint32))), None, total)
    opart.update_batch(v, g, None, total)
    st = [s.to_arrow() for s in part.state()]
    for s, os_ in zip(st, opart.state()):
        assert same_arrow(s, os_)
    perm = rng.permutation(total)
    filt = pa.array(rng.random(total) < 0.8)
    views_ = []
    for s in st:          # a state column is a view of class A (no NULL in it) or C (the sums of groups nothing was added to are NULL) at the rows the class names
        nullable = s.null_count > 0
        off = 64 if (nullable or cls != "A-odd-rows") else 3
        views_.append(ViewCase("s", off, total, "some" if nullable else "none").make(ctx, None, rng, arr=s)[0])
    pv, _ = ViewCase("g", 1, total).make(ctx, "uint32", rng, arr=pa.array(perm.astype(np.uint32)))
    fv, _ = ViewCase("f", 128, total).make(ctx, "bool", rng, arr=filt)
    a, o = new_acc(ctx, fun, v); b, _ = new_acc(ctx, fun, v)
    for use_filter in (False, True):
        a.merge_batch(views_, pv, fv if use_filter else None, total)
        b.merge_batch([ctx.from_arrow(s) for s in st], ctx.from_arrow(pa.array(perm.astype(np.uint32))), ctx.from_arrow(filt) if use_filter else None, total)
        o.merge_batch(st, perm, filt if use_filter else None, total)
    assert_acc_equal(a, b, o)


FUSED_NODES = [("column", 0, 0), ("column", 1, 0), ("scalar", 2, 0), ("-", 2, 1), ("*", 0, 3)]          # x * (1 - y)


@pytest.mark.parametrize("money", ["quarters", "decimal"])
@pytest.mark.parametrize("off", [1, 3, 64, 65])
def test_update_batch_fused_over_views_succeeds_or_reports_not_implemented(ctx, money, off):
    """dfgpu_acc_update_batch_fused loads its columns with 16-byte vector loads and answers NOT_IMPLEMENTED -- with nothing accumulated -- for a column that is not 16-byte
    aligned: a Float64 view at an odd row.  A Decimal128 view is aligned at every row and is taken.  Either way the accumulators end as node-by-node evaluation leaves them;
    the plan-level test below shows the operator's fallback."""
    import dfgpu
    rng = rng_for("fused", money, off)
    n, total = 50001, 6
    if money == "decimal":
        mk = lambda lo, hi: pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(lo, hi, n)], type=pa.decimal128(15, 2))
        one, T, tp = pa.array([decimal.Decimal(1)], type=pa.decimal128(20, 0)), dfgpu.capi.DECIMAL128, [(38, 4), (15, 2)]
    else:
        mk = lambda lo, hi: pa.array(rng.integers(lo, hi, n) * 0.25)
        one, T, tp = pa.array([1.0]), dfgpu.capi.FLOAT64, [(0, 0), (0, 0)]
    x, y = mk(0, 4000), mk(0, 9)
    g = rng.integers(0, total, n).astype(np.uint32)
    xv, _ = ViewCase("x", off, n).make(ctx, None, rng, arr=x)
    yv, _ = ViewCase("y", off, n).make(ctx, None, rng, arr=y)
    gd, od = ctx.from_arrow(pa.array(g)), ctx.from_arrow(one)
    make = lambda: [dfgpu.GroupsAccumulator(ctx, KIND["SUM"], T, *tp[0]), dfgpu.GroupsAccumulator(ctx, KIND["AVG"], T, *tp[1]), dfgpu.GroupsAccumulator(ctx, KIND["COUNT"], dfgpu.capi.INT64)]
    fused, plain_ = make(), make()
    expect_taken = not misaligned(xv)
    assert expect_taken == (money == "decimal" or off % 2 == 0)
    try:
        dfgpu.GroupsAccumulator.update_batch_fused(ctx, fused, [4, 1, -1], FUSED_NODES, [xv, yv, od], gd, None, total)
        taken = True
    except dfgpu.DfgpuError as e:
        assert e.kind == "NotImplemented", e
        taken = False
    assert taken == expect_taken
    price = ctx.binary(2, xv, ctx.binary(1, od, yv, lhs_scalar=True))
    if not taken:          # nothing was accumulated: the caller's fallback, node by node
        dfgpu.GroupsAccumulator.update_batch_multi(ctx, fused, [price, yv, None], [None] * 3, gd, total)
    dfgpu.GroupsAccumulator.update_batch_multi(ctx, plain_, [ctx.binary(2, ctx.from_arrow(x), ctx.binary(1, od, ctx.from_arrow(y), lhs_scalar=True)), ctx.from_arrow(y), None], [None] * 3, gd, total)
    want_price = po.binary("*", x, po.binary("-", one, y, l_scalar=True))
    assert same_arrow(price.to_arrow(), want_price)
    oaccs = [po.Acc("SUM", want_price.type), po.Acc("AVG", y.type), po.Acc("COUNT", pa.int64())]
    for o, col in zip(oaccs, (want_price, y, None)):
        o.update_batch(col, g.astype(np.int64), None, total)
    for a, b, o in zip(fused, plain_, oaccs):
        assert_acc_equal(a, b, o)


def test_group_values_intern_of_odd_row_dictionary_views_feeds_the_accumulators(ctx):
    """class D: two non-null dictionary key columns whose Int32 codes are views.  The dense code-tuple map of groups.hip builds its first-row table with 16-byte loads of the
    codes and is gated on their alignment: at row 1 the codes are 4 but not 16 bytes aligned and k_dense_first_fast runs in place of k_dense_first_tab (the profile shows which).  The ids -- also as a deferred recipe, which
    dfgpu_acc_update_batch_fused evaluates itself only over aligned code columns and materialises otherwise -- drive the accumulators exactly as the oracle's ids do."""
    import dfgpu
    rng = rng_for("intern")
    n = 40001
    k1 = pa.array(np.array(["A", "N", "R"], dtype=object)[rng.integers(0, 3, n)], type=pa.utf8()).dictionary_encode()
    k2 = pa.array(np.array(["F", "O"], dtype=object)[rng.integers(0, 2, n)], type=pa.utf8()).dictionary_encode()
    v = acc_values("int64", n, True, rng)
    x, y, one = pa.array(rng.integers(0, 4000, n) * 0.25), pa.array(rng.integers(0, 9, n) * 0.25), pa.array([1.0])
    og = po.Groups([k1.type, k2.type]); oids = og.intern([k1, k2]); total = len(og)
    osum = po.Acc("SUM", v.type); osum.update_batch(v, oids, None, total)
    price = po.binary("*", x, po.binary("-", one, y, l_scalar=True))
    oprice = po.Acc("SUM", pa.float64()); oprice.update_batch(price, oids, None, total)
    for off in (1, 64):
        kv = [ViewCase("k1", off, n).make(ctx, "dict", rng, arr=k1)[0], ViewCase("k2", off, n).make(ctx, "dict", rng, arr=k2)[0]]
        assert misaligned(kv[0]) == (off == 1) and misaligned(kv[1]) == (off == 1)
        for deferred in (False, True):
            gv = dfgpu.GroupValues(ctx, 2)
            gids, ks = profiled(ctx, lambda: gv.intern(kv, deferred=deferred))
            assert "k_groups_dense" in ks and ("k_dense_first_fast" in ks) == (off == 1) and ("k_dense_first_tab" in ks) == (off == 64), ks
            assert len(gv) == total
            acc, _ = new_acc(ctx, "SUM", v)
            acc.update_batch(ctx.from_arrow(v), gids, None, total)
            fused = [dfgpu.GroupsAccumulator(ctx, KIND["SUM"], dfgpu.capi.FLOAT64)]
            dfgpu.GroupsAccumulator.update_batch_fused(ctx, fused, [4], FUSED_NODES, [ctx.from_arrow(x), ctx.from_arrow(y), ctx.from_arrow(one)], gids, None, total)
            assert np.array_equal(gids.to_numpy().astype(np.int64), oids)
            assert same_arrow(acc.evaluate().to_arrow(), osum.evaluate()) and same_arrow(fused[0].evaluate().to_arrow(), oprice.evaluate())
            for a, w in zip(gv.emit(), og.emit()):
                assert same_arrow(a.to_arrow(), w)


# ------------------------------------------------------------------ concat
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "dict"])
def test_concat_of_views_then_slice_and_export(ctx, kind):
    """parts: a view at an odd row (class A / B, or E), a view of a view, a zero-length view in the middle, a class C view with a ragged last word, a whole-parent view;
    the Utf8 parts each start at offsets[0] > 0 over a values buffer that is the parent's"""
    rng = rng_for("concat", kind)
    cases = [ViewCase("odd", 3, 100), ViewCase("vv", 64, 37, "some", off2=64), ViewCase("empty", 77, 0, tail=0), ViewCase("ragged", 128, 961, "some"),
             ViewCase("vv-odd", 1, 65, off2=2), ViewCase("whole", 0, 130, "some", tail=0), ViewCase("only-nulls", 64, 63, "all")]
    made = [c.make(ctx, kind, rng) for c in cases]
    cat = ctx.concat([v for v, _ in made])
    want = pa.concat_arrays([e for _, e in made])
    base = ctx.concat([ctx.from_arrow(e) for _, e in made])
    assert same_arrow(cat.to_arrow(), want) and same_arrow(cat.to_arrow(), base.to_arrow())
    assert cat.null_count == want.null_count
    total = len(want)
    for off, ln in [(0, 64), (64, 500), (3, 70), (100, 37), (137, 0), (total - 1, 1), (total, 0), (128, total - 128)]:
        s = cat.slice(off, ln)
        assert same_arrow(s.to_arrow(), want.slice(off, ln)) and s.null_count == want.slice(off, ln).null_count
        again = ctx.concat([s, cat.slice(0, 5), s])          # views of the concatenation, concatenated again
        assert same_arrow(again.to_arrow(), pa.concat_arrays([want.slice(off, ln), want.slice(0, 5), want.slice(off, ln)]))


def test_concat_of_dictionary_views_of_one_parent(ctx):
    """class D: concat takes dictionary arrays that share one dictionary -- windows of one parent do"""
    rng = rng_for("concat-dict")
    col = rand_array("dict", 3000, 0.2, rng)
    parent = ctx.from_arrow(col)
    parts = [(64, 961), (1024, 0), (1, 100), (1088, 1023), (0, 3000)]
    vs = [parent.slice(o, n) for o, n in parts]
    for (o, n), v in zip(parts, vs):
        assert views.is_view(parent, v, o) == (o % 64 == 0)
    cat = ctx.concat(vs)
    want = pa.concat_arrays([col.slice(o, n) for o, n in parts])
    assert same_arrow(cat.to_arrow(), want) and cat.null_count == want.null_count
    assert same_arrow(cat.slice(961, 100).to_arrow(), want.slice(961, 100))


# ------------------------------------------------------------------ plans over batches of views
def view_batch(ctx, table, off, rng, nullable=()):
    """RecordBatch whose columns are windows at row `off` of larger parents; `nullable`: names of the columns that carry validity"""
    from dfgpu import physical_plan as ops
    cols = []
    for name in table.column_names:
        arr = table[name].combine_chunks()
        v, _ = ViewCase(name, off, len(arr), "some" if name in nullable else "none").make(ctx, None, rng, arr=arr)
        cols.append(v)
    batch = ops.RecordBatch.from_arrays(ctx, table.column_names, cols)
    batch.view_columns = cols
    return batch


def run_plan(plan, ctx):
    from dfgpu import physical_plan as ops
    out = [b.to_arrow() for b in ops.collect(plan, ops.TaskContext(ctx, 8192))]
    return pa.concat_tables(out) if out else None


def rows_sorted(t):
    from helpers import rows_of, sort_rows
    return sort_rows(rows_of([t.column(i) for i in range(t.num_columns)]))


PLAN_OFFS = [(1, 9001), (64, 8961), (128, 9023)]          # an odd row; multiples of 64 with a ragged length


def plan_tables(rng, n):
    t = pa.table({"k": pa.array(rng.integers(0, 6, n).astype(np.int64)), "d": pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(-10**9, 10**9, n)], type=pa.decimal128(15, 2)),
                  "x": pa.array(rng.integers(0, 4000, n) * 0.25), "y": pa.array(rng.integers(0, 9, n) * 0.25), "c": pa.array(rng.integers(0, 40, n).astype(np.int64), mask=rng.random(n) < 0.1),
                  "s": pa.array([f"s{i % 11}" for i in rng.integers(0, 1000, n)], type=pa.utf8())})
    return t


@pytest.mark.parametrize("off,n", PLAN_OFFS)
def test_filter_projection_aggregate_plan_over_view_batches(ctx, off, n):
    """MemoryExec (two batches of views) -> FilterExec -> ProjectionExec -> AggregateExec Single: SUM(Decimal128), AVG(Decimal128), COUNT(DISTINCT c), MIN(s) by k.
    Equal to the same plan over materialised batches and to the oracle's accumulators over the filtered rows."""
    import dfgpu
    from dfgpu import physical_plan as ops
    rng = rng_for("plan-agg", off)
    tabs = [plan_tables(rng, n), plan_tables(rng, n // 2 + 1)]
    C, L, B, F = ops.Column, ops.Literal, ops.BinaryExpr, ops.Field

    def plan(batches):
        src = ops.MemoryExec([batches], batches[0].schema)
        f = ops.FilterExec(B(C("x", 2), "<", L(700.0, pa.float64())), src)
        pj = ops.ProjectionExec([(C("k", 0), "k"), (C("d", 1), "d"), (C("c", 4), "c"), (C("s", 5), "s")], f)
        aggs = [ops.AggregateFunctionExpr("SUM", C("d", 1), "sum_d", input_field=F("d", dfgpu.capi.DECIMAL128, 15, 2)), ops.AggregateFunctionExpr("AVG", C("d", 1), "avg_d", input_field=F("d", dfgpu.capi.DECIMAL128, 15, 2)),
                ops.AggregateFunctionExpr("COUNT DISTINCT", C("c", 2), "cd", input_field=F("c", dfgpu.capi.INT64)), ops.AggregateFunctionExpr("MIN", C("s", 3), "min_s", input_field=F("s", dfgpu.capi.UTF8))]
        return ops.AggregateExec("Single", [(C("k", 0), "k")], aggs, pj)
    got = run_plan(plan([view_batch(ctx, t, off, rng, nullable=("c",)) for t in tabs]), ctx)
    base = run_plan(plan([ops.batch_from_arrow(ctx, t) for t in tabs]), ctx)
    assert rows_sorted(got) == rows_sorted(base) and [c.type for c in got.columns] == [c.type for c in base.columns]
    whole = pa.concat_tables(tabs)
    keep = po.binary("<", whole["x"].combine_chunks(), pa.array([700.0]), r_scalar=True)
    t = pa.table([po.filter_(whole[c].combine_chunks(), keep) for c in whole.column_names], names=whole.column_names)
    og = po.Groups([pa.int64()]); gids = og.intern([t["k"].combine_chunks()]); total = len(og)
    s, a = po.Acc("SUM", t["d"].type), po.Acc("AVG", t["d"].type)
    s.update_batch(t["d"].combine_chunks(), gids, None, total); a.update_batch(t["d"].combine_chunks(), gids, None, total)
    cd = po.count_distinct(t["c"].combine_chunks(), gids, total)
    ms = po.string_min_max(t["s"].combine_chunks(), gids, total, False)
    want = pa.table([og.emit()[0], s.evaluate(), a.evaluate(), pa.array(cd, type=pa.int64()) if not isinstance(cd, pa.Array) else cd, ms], names=["k", "sum_d", "avg_d", "cd", "min_s"])
    assert rows_sorted(got) == rows_sorted(want)


@pytest.mark.parametrize("off,n", PLAN_OFFS)
def test_fused_aggregate_plan_falls_back_for_a_misaligned_view_batch(ctx, off, n):
    """SUM(x * (1 - y)), AVG(y), COUNT(*) over a projection: the aggregate looks through the projection and hands the expression to dfgpu_acc_update_batch_fused.  A batch of
    Float64 views at an odd row is not 16-byte aligned: the call answers NOT_IMPLEMENTED and AggregateExec evaluates the arguments node by node (k_acc_fused absent from the
    profile); at a multiple of 64 rows the fused kernel runs.  The values are multiples of 1/4, so every sum is exact whatever the order of the additions."""
    import dfgpu
    from dfgpu import physical_plan as ops
    rng = rng_for("plan-fused", off)
    tabs = [plan_tables(rng, n).select(["k", "x", "y"])]
    C, L, B, F = ops.Column, ops.Literal, ops.BinaryExpr, ops.Field

    def plan(batches):
        src = ops.MemoryExec([batches], batches[0].schema)
        pj = ops.ProjectionExec([(B(C("x", 1), "*", B(L(1.0, pa.float64()), "-", C("y", 2))), "price"), (C("y", 2), "y"), (C("k", 0), "k")], src)
        aggs = [ops.AggregateFunctionExpr("SUM", C("price", 0), "sum_price", input_field=F("p", dfgpu.capi.FLOAT64)), ops.AggregateFunctionExpr("AVG", C("y", 1), "avg_y", input_field=F("y", dfgpu.capi.FLOAT64)),
                ops.AggregateFunctionExpr("COUNT", None, "n")]
        return ops.AggregateExec("Single", [(C("k", 2), "k")], aggs, pj)
    saved = ctx.get_option("fused_aggregate_min_rows")
    ctx.set_option("fused_aggregate_min_rows", 0)
    ctx.profile_select(None); ctx.profile_enable(True); ctx.profile_read()
    try:
        vb = view_batch(ctx, tabs[0], off, rng)
        assert misaligned(vb.view_columns[1]) == (off % 2 == 1)
        got = run_plan(plan([vb]), ctx)
        ks = set(ctx.profile_read())
        base = run_plan(plan([ops.batch_from_arrow(ctx, tabs[0])]), ctx)
        kb = set(ctx.profile_read())
    finally:
        ctx.profile_enable(False); ctx.set_option("fused_aggregate_min_rows", saved)
    assert ("k_acc_fused" in ks) == (off % 2 == 0), ks
    assert "k_acc_fused" in kb, kb
    assert rows_sorted(got) == rows_sorted(base)
    t = tabs[0]
    price = po.binary("*", t["x"].combine_chunks(), po.binary("-", pa.array([1.0]), t["y"].combine_chunks(), l_scalar=True))
    og = po.Groups([pa.int64()]); gids = og.intern([t["k"].combine_chunks()]); total = len(og)
    s, a, c = po.Acc("SUM", pa.float64()), po.Acc("AVG", pa.float64()), po.Acc("COUNT", pa.int64())
    s.update_batch(price, gids, None, total); a.update_batch(t["y"].combine_chunks(), gids, None, total); c.update_batch(None, gids, None, total)
    want = pa.table([og.emit()[0], s.evaluate(), a.evaluate(), c.evaluate()], names=["k", "s", "a", "c"])
    assert rows_sorted(got) == rows_sorted(want)


@pytest.mark.parametrize("off,n", PLAN_OFFS)
def test_sort_exec_with_fetch_over_view_batches(ctx, off, n):
    from dfgpu import physical_plan as ops
    rng = rng_for("plan-sort", off)
    tabs = [plan_tables(rng, n), plan_tables(rng, 777)]

    def plan(batches):
        return ops.SortExec([ops.PhysicalSortExpr(ops.Column("c", 4), True, False), ops.PhysicalSortExpr(ops.Column("d", 1), False, True)], ops.MemoryExec([batches], batches[0].schema), fetch=1000)
    got = run_plan(plan([view_batch(ctx, t, off, rng, nullable=("c",)) for t in tabs]), ctx)
    base = run_plan(plan([ops.batch_from_arrow(ctx, t) for t in tabs]), ctx)
    whole = pa.concat_tables(tabs).combine_chunks()
    order = po.lexsort_to_indices([whole["c"].combine_chunks(), whole["d"].combine_chunks()], [True, False], [False, True])[:1000]
    assert got.equals(base) and got.equals(whole.take(pa.array(order)))


@pytest.mark.parametrize("off,n", PLAN_OFFS)
def test_hash_join_exec_with_view_batches_on_both_sides(ctx, off, n):
    from dfgpu import physical_plan as ops
    rng = rng_for("plan-join", off)
    left = pa.table({"k": pa.array(rng.permutation(np.arange(3000, dtype=np.int64) * 2)), "pay": pa.array(rng.integers(0, 10**6, 3000)), "s": pa.array([f"b{i % 97}" for i in range(3000)])})
    right = pa.table({"k": pa.array(rng.integers(0, 7000, n).astype(np.int64), mask=rng.random(n) < 0.05), "w": pa.array(rng.integers(0, 100, n))})

    def plan(lb, rb):
        return ops.HashJoinExec(ops.MemoryExec([[lb]], lb.schema), ops.MemoryExec([[rb]], rb.schema), [(ops.Column("k", 0), ops.Column("k", 0))], None, "Inner", "CollectLeft")
    got = run_plan(plan(view_batch(ctx, left, off + 2 if off % 2 else off, rng), view_batch(ctx, right, off, rng, nullable=("k",))), ctx)
    base = run_plan(plan(ops.batch_from_arrow(ctx, left), ops.batch_from_arrow(ctx, right)), ctx)
    want = po.hash_join([[left["k"].combine_chunks()]], [[right["k"].combine_chunks()]], "Inner", False, batch_size=1 << 40)
    wt = pa.table([left[c].combine_chunks().take(pa.array(want.build_idx)) for c in left.column_names] + [right[c].combine_chunks().take(pa.array(want.probe_idx)) for c in right.column_names],
                  names=["k", "pay", "s", "k2", "w"])
    assert rows_sorted(got) == rows_sorted(base) == rows_sorted(wt) and got.num_rows > 100
