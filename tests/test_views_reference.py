"""No GPU: the references that tests/test_gpu_views.py compares against are well defined on a window, and tests/views.py builds what it says.

For every operator of the device tests, the oracle over `parent.slice(off, n)` (pyarrow's own zero-copy slice of the parent that the device tests import)
equals the oracle over the materialised window, for every kind and every view case; and the parents hold the window unchanged between adversarial rows."""
import numpy as np
import pyarrow as pa
import pytest

import views
from oracle import pyoracle as po
from test_gpu_core import KINDS
from test_gpu_expr import CASTS, CMP, same
from views import VIEW_CASES, plain


def ids(cases):
    return [c.id for c in cases]


def windows(case, kind, seed=0):
    """(window sliced out of the parent, window built on its own)"""
    parent, off, arr = case.host(kind, np.random.default_rng([seed, len(kind), case.off, case.n]))
    return parent.slice(off, len(arr)), arr


def eq(a, b):
    return same(plain(a), plain(b))


@pytest.mark.parametrize("case", VIEW_CASES, ids=ids(VIEW_CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_parent_holds_the_window_between_adversarial_rows(kind, case):
    parent, off, arr = case.host(kind, np.random.default_rng(5))
    n = len(arr)
    assert parent.type == arr.type or pa.types.is_dictionary(arr.type)
    assert eq(parent.slice(off, n), arr) and parent.slice(off, n).null_count == arr.null_count
    assert (parent.null_count > 0) == case.nullable          # class A / B parents carry no validity, class C / E parents do
    outside = pa.concat_arrays([plain(parent.slice(0, off)), plain(parent.slice(off + n))])
    assert len(outside) == len(parent) - n
    assert outside.null_count == (1 if case.nullable and arr.null_count == 0 else 0)          # valid bits are set (one NULL row gives a NULL-free window its validity buffer)
    vals = outside.drop_null().to_pylist() if kind != "date32" else outside.cast(pa.int32()).drop_null().to_pylist()
    if kind == "bool":
        assert all(vals)
    elif kind in ("utf8", "dict"):
        assert all(len(s) > 0 for s in vals)
    if kind == "dict" and len(parent) > n:
        inside = set(arr.indices.drop_null().to_pylist())
        pad_codes = set(parent.indices.slice(0, off).drop_null().to_pylist()) | set(parent.indices.slice(off + n).drop_null().to_pylist())
        assert pad_codes and not (pad_codes & inside) and max(pad_codes) < len(parent.dictionary)
    if kind in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64") and len(vals) > 8:
        info = np.iinfo(arr.type.to_pandas_dtype())
        assert info.max in vals and info.min in vals                                           # extremes ...
        if n and arr.null_count < n:
            assert set(vals) & set(arr.drop_null().to_pylist())                                # ... and values that also occur inside the window


def test_is_view_decides_from_the_descriptors():
    """is_view over stand-ins for Array.describe(): pointer arithmetic per type, no device needed"""
    from types import SimpleNamespace as D

    class A:
        def __init__(self, **kw):
            self.d = D(**{**dict(type=5, key_type=0, values=None, validity=None, offsets=None), **kw})

        def describe(self):
            return self.d
    assert views.is_view(A(values=4096), A(values=4096 + 8 * 3), 3) and not views.is_view(A(values=4096), A(values=8192), 3)
    assert views.is_view(A(type=2, values=4096), A(type=2, values=4097), 1)
    assert views.is_view(A(values=4096, validity=512), A(values=4096 + 512, validity=520), 64) and not views.is_view(A(values=4096, validity=512), A(values=4096 + 512, validity=1024), 64)
    assert not views.is_view(A(values=4096, validity=512), A(values=4096 + 512), 64)
    assert views.is_view(A(type=14, values=4096, offsets=256), A(type=14, values=4096, offsets=260), 1) and not views.is_view(A(type=14, values=4096, offsets=256), A(type=14, values=5000, offsets=260), 1)
    assert views.is_view(A(type=1, values=4096), A(type=1, values=4104), 64) and not views.is_view(A(type=1, values=4096), A(type=1, values=4096), 3)
    assert views.is_view(A(type=15, key_type=4, values=4096), A(type=15, key_type=4, values=4100), 1)


@pytest.mark.parametrize("case", VIEW_CASES, ids=ids(VIEW_CASES))
@pytest.mark.parametrize("kind", KINDS)
def test_hash_take_filter_references_on_a_window(kind, case):
    w, a = windows(case, kind)
    n = len(a)
    assert np.array_equal(po.create_hashes([w]), po.create_hashes([a]))
    rng = np.random.default_rng(n + 1)
    idx = rng.integers(0, max(n, 1), 300 if n else 0)
    assert eq(po.take(w, idx), po.take(a, idx)) and eq(po.take(a, idx), plain(a).take(pa.array(idx)))
    m = pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.1)
    assert eq(po.filter_(w, m), po.filter_(a, m)) and eq(po.filter_(a, m), plain(a).filter(m, null_selection_behavior="drop"))


@pytest.mark.parametrize("case", VIEW_CASES, ids=ids(VIEW_CASES))
@pytest.mark.parametrize("kind", ["int16", "int64", "float64", "decimal", "utf8", "bool"])
def test_expression_references_on_a_window(kind, case):
    lw, la = windows(case, kind, 1)
    rw, ra = windows(case, kind, 2)
    ops = CMP + {"bool": ["AND", "OR"], "utf8": []}.get(kind, ["+", "-", "*"])
    for op in ops:
        assert eq(po.binary(op, lw, rw), po.binary(op, la, ra)), op
        s = pa.concat_arrays([ra.drop_null().slice(0, 1), ra.slice(0, 0)]) if ra.null_count < len(ra) else None
        if s is not None:
            assert eq(po.binary(op, lw, s, r_scalar=True), po.binary(op, la, s, r_scalar=True)), op
    for neg in (False, True):
        assert eq(po.is_null(lw, neg), po.is_null(la, neg))
    if kind == "bool":
        assert eq(po.not_(lw), po.not_(la))
    if kind in ("int64", "float64", "decimal"):
        assert eq(po.negative(lw), po.negative(la))
    if kind == "int64":
        for lst in [pa.array([1, 5, 7]), pa.array([1, None, 7]), pa.array([], type=pa.int64())]:
            assert eq(po.in_list(lw, lst, True), po.in_list(la, lst, True))


@pytest.mark.parametrize("case", views.VIEW_CASES_SHORT, ids=ids(views.VIEW_CASES_SHORT))
@pytest.mark.parametrize("kind,to", [c for c in CASTS if c[1] is not None], ids=[f"{k}-to-{t}" for k, t in CASTS if t is not None])
def test_cast_reference_on_a_window(kind, to, case):
    w, a = windows(case, kind)
    assert eq(po.cast(w, to), po.cast(a, to))


@pytest.mark.parametrize("case", VIEW_CASES, ids=ids(VIEW_CASES))
def test_sort_partition_join_and_accumulator_references_on_a_window(case):
    (w1, a1), (w2, a2), (wu, au) = windows(case, "int32", 1), windows(case, "int64", 2), windows(case, "utf8", 3)
    n = len(a1)
    for desc, nf in (([False, True, False], [True, False, True]), ([True, False, True], [False, True, False])):
        got = po.lexsort_to_indices([w1, wu, w2], desc, nf)
        assert np.array_equal(got, po.lexsort_to_indices([a1, au, a2], desc, nf))
    for nparts in (3, 64):
        (i1, c1), (i2, c2) = po.hash_partition([w1, w2], nparts), po.hash_partition([a1, a2], nparts)
        assert np.array_equal(i1, i2) and np.array_equal(c1, c2)
    if n:
        j1, j2 = po.hash_join([[w2]], [[w2]], "Inner", False, batch_size=1 << 40), po.hash_join([[a2]], [[a2]], "Inner", False, batch_size=1 << 40)
        assert np.array_equal(j1.build_idx, j2.build_idx) and np.array_equal(j1.probe_idx, j2.probe_idx)
        ju, ja = po.hash_join([[wu]], [[wu]], "Inner", False, batch_size=1 << 40), po.hash_join([[au]], [[au]], "Inner", False, batch_size=1 << 40)
        assert np.array_equal(ju.probe_idx, ja.probe_idx)
    g = np.random.default_rng(n).integers(0, 7, n)
    for fun, (w, a) in (("SUM", (w2, a2)), ("AVG", windows(case, "decimal", 4)), ("MIN", (w1, a1)), ("COUNT", (wu, au))):
        x, y = po.Acc(fun, a.type), po.Acc(fun, a.type)
        x.update_batch(w, g, None, 7); y.update_batch(a, g, None, 7)
        assert eq(x.evaluate(), y.evaluate())
        for s, t in zip(x.state(), y.state()):
            assert eq(s, t)
        z = po.Acc(fun, a.type)
        z.merge_batch(x.state(), np.arange(7), None, 7)
        assert eq(z.evaluate(), y.evaluate())
    og1, og2 = po.Groups([a1.type, au.type]), po.Groups([a1.type, au.type])
    assert np.array_equal(og1.intern([w1, wu]), og2.intern([a1, au]))
    assert eq(pa.concat_arrays([w1, w1.slice(0, 0), w1]), pa.concat_arrays([a1, a1]))


@pytest.mark.parametrize("case", VIEW_CASES, ids=ids(VIEW_CASES))
def test_mask_dictionary_literal_in_list_and_fused_expression_references_on_a_window(case):
    """the remaining references of the device tests: mask_to_indices / mask_count (numpy over the Boolean window), a dictionary column against a literal (the oracle over the
    decoded column), in_list over Utf8, and the expression the fused accumulator update evaluates, x * (1 - y)"""
    mw, ma = windows(case, "bool", 1)
    truth = lambda m: np.asarray(m.fill_null(False), dtype=bool)
    assert np.array_equal(np.flatnonzero(truth(mw)), np.flatnonzero(truth(ma))) and int(truth(mw).sum()) == int(truth(ma).sum())
    dw, da = windows(case, "dict", 2)
    lit = pa.array(["BUILDING0"], type=pa.utf8())
    assert dw.dictionary is not da.dictionary and len(dw.dictionary) == len(da.dictionary) + 2          # the window out of the parent drags the parent's dictionary along
    for op in CMP:
        assert eq(po.binary(op, dw.cast(pa.utf8()), lit, r_scalar=True), po.binary(op, da.cast(pa.utf8()), lit, r_scalar=True)), op
        assert eq(po.binary(op, lit, dw.cast(pa.utf8()), l_scalar=True), po.binary(op, lit, da.cast(pa.utf8()), l_scalar=True)), op
    uw, ua = windows(case, "utf8", 3)
    lst = pa.array(["BUILDING0", "ASIA3", "a1"])
    for neg in (False, True):
        assert eq(po.in_list(uw, lst, neg), po.in_list(ua, lst, neg))
    rng = np.random.default_rng(case.n + 7)
    one = pa.array([1.0])
    x, y = pa.array(rng.integers(0, 4000, case.n) * 0.25), pa.array(rng.integers(0, 9, case.n) * 0.25)
    (px, ox, _), (py, oy, _) = case.host(None, rng, arr=x), case.host(None, rng, arr=y)
    price = lambda a, b: po.binary("*", a, po.binary("-", one, b, l_scalar=True))
    assert eq(price(px.slice(ox, case.n), py.slice(oy, case.n)), price(x, y))
    g = rng.integers(0, 6, case.n)
    s1, s2 = po.Acc("SUM", pa.float64()), po.Acc("SUM", pa.float64())
    s1.update_batch(price(px.slice(ox, case.n), py.slice(oy, case.n)), g, None, 6); s2.update_batch(price(x, y), g, None, 6)
    assert eq(s1.evaluate(), s2.evaluate())

