"""Array views for the parity tests: windows into a larger parent array, as dfgpu_array_slice hands them out.

A view shares its parent's buffers, so it breaks what holds for a freshly imported array (include/dfgpu.h, "What a consumer of a
dfgpu_array may assume"):

  A  non-null fixed-width column, any row offset      values aligned to the element width only
  B  non-null Utf8, any row offset                    offsets[0] > 0, values = the parent's base, values_bytes an upper bound
  C  validity or Boolean values, offset % 64 == 0     bits past `length` in the last word are the parent's live bits, null_count == -1
  D  dictionary column                                codes follow A or C, the dictionary is the parent's
  E  validity or Boolean values, offset % 64 != 0     a copy through take, not a view: the control arm

`parent_arrow` builds the parent on the host (the CPU tests use it alone), `as_view` imports it and slices, `is_view` decides from
Array.describe() whether a slice really is a view.  The rows around the window are adversarial: a kernel that reads a row, a word or a
byte outside the window finds valid bits, true Booleans, extreme numbers that also occur inside the window, non-empty strings and valid
dictionary codes there -- never a zero that would hide the read."""
import decimal
from dataclasses import dataclass

import numpy as np
import pyarrow as pa

from test_gpu_core import rand_array

# dfgpu_type ids (include/dfgpu.h) -> element width in bytes; Boolean and Utf8 have none
BOOL, UTF8, DICTIONARY = 1, 14, 15
WIDTH = {2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 2, 8: 4, 9: 8, 10: 4, 11: 8, 12: 4, 13: 16}
TAIL = 70          # more than one bitmap word: the window's last word is shared with pad rows only


def plain(a):
    return a.dictionary_decode() if pa.types.is_dictionary(a.type) else a


def _extremes(t):
    if pa.types.is_boolean(t):
        return [True]
    if pa.types.is_integer(t):
        i = np.iinfo(t.to_pandas_dtype())
        return [int(i.max), int(i.min)]
    if pa.types.is_date32(t):
        return [2**31 - 1, -2**31]
    if pa.types.is_floating(t):
        f = np.finfo(t.to_pandas_dtype())
        return [float("inf"), float("-inf"), float(f.max), float("nan")]
    if pa.types.is_decimal(t):
        top = decimal.Decimal(10**t.precision - 1).scaleb(-t.scale)
        return [top, -top]
    if t == pa.utf8():
        return ["\x7f" * 19, "PAD"]
    raise ValueError(t)


def pad_rows(arr, n, poison=True, salt=0):
    """n all-valid rows of arr's type to put around the window.  poison: the type's extremes and values taken from the window, in turn; else zeros."""
    t = arr.type
    if pa.types.is_dictionary(t):
        raise ValueError("dictionary parents are assembled in parent_arrow")
    if not poison:
        pool = ["x"] if t == pa.utf8() else [False] if pa.types.is_boolean(t) else [decimal.Decimal(0)] if pa.types.is_decimal(t) else [0]
    else:
        win = arr.cast(pa.int32()) if pa.types.is_date32(t) else arr
        inside = [] if pa.types.is_boolean(t) else [v for v in win.drop_null().slice(0, 6).to_pylist() if v != ""]
        ex, pool = _extremes(t), []
        for i in range(max(len(ex), len(inside))):
            pool += [ex[i % len(ex)]] + ([inside[i % len(inside)]] if inside else [])
    vals = [pool[(i + salt) % len(pool)] for i in range(n)]
    if pa.types.is_date32(t):
        return pa.array(vals, type=pa.int32()).cast(pa.date32())
    return pa.array(vals, type=t)


def parent_arrow(arr, off, tail=TAIL, poison=True, force_validity=False):
    """`off` pad rows, then `arr`, then `tail` pad rows; force_validity makes the first pad row NULL (the row behind the tail when there is no pad), so
    that the parent carries a validity buffer although the window may hold no NULL; a view starts on a bitmap word of its own, so that row
    never shares a word with the window.  parent.slice(off, len(arr)) equals arr."""
    if pa.types.is_dictionary(arr.type):
        # pad codes are valid and differ from every code of the window: they point at two entries appended to the dictionary
        vt, nd = arr.type.value_type, len(arr.dictionary)
        extra = pa.array(["PAD_LO", "PAD_HI"], type=vt) if vt == pa.utf8() else pad_rows(pa.array([], type=vt), 2)
        codes = np.array([nd + (i & 1) for i in range(off + tail)], dtype=arr.type.index_type.to_pandas_dtype())
        it = arr.type.index_type
        head = pa.array(codes[:off]) if not (force_validity and off) else pa.concat_arrays([pa.nulls(1, it), pa.array(codes[1:off])])
        idx = pa.concat_arrays([head, arr.indices, pa.array(codes[off:])] + ([pa.nulls(1, it)] if force_validity and not off else []))
        return pa.DictionaryArray.from_arrays(idx, pa.concat_arrays([arr.dictionary, extra]))
    head = pad_rows(arr, off, poison, 0) if not (force_validity and off) else pa.concat_arrays([pa.nulls(1, arr.type), pad_rows(arr, off - 1, poison, 0)])
    parts = [head, arr, pad_rows(arr, tail, poison, 1)] + ([pa.nulls(1, arr.type)] if force_validity and not off else [])
    return pa.concat_arrays(parts)


def as_view(ctx, arr, off, tail=TAIL, poison=True, force_validity=False):
    """-> (view, expected): the window [off, off + len(arr)) of an imported parent, and `arr` itself.  view.parent / view.off serve is_view."""
    parent = ctx.from_arrow(parent_arrow(arr, off, tail, poison, force_validity))
    view = parent.slice(off, len(arr))
    view.parent, view.off = parent, off
    return view, arr


def view_of_view(ctx, arr, off1, off2, force_validity=False):
    """the same window reached through two slices: parent.slice(off1, ..).slice(off2, len(arr))"""
    parent = ctx.from_arrow(parent_arrow(arr, off1 + off2, TAIL, True, force_validity))
    mid = parent.slice(off1, off2 + len(arr) + TAIL // 2)
    view = mid.slice(off2, len(arr))
    view.parent, view.off = parent, off1 + off2
    return view, arr


def is_view(parent, view, off):
    """Array.describe() of both: every buffer of `view` is the parent's buffer moved on by `off` rows (no copy was made)."""
    p, v = parent.describe(), view.describe()
    if p.type != v.type or (p.validity is None) != (v.validity is None):
        return False
    vt = p.key_type if p.type == DICTIONARY else p.type
    if p.type == UTF8:
        ok = (v.offsets or 0) == (p.offsets or 0) + 4 * off and v.values == p.values
    elif vt == BOOL:
        ok = off % 8 == 0 and (v.values or 0) == (p.values or 0) + off // 8
    else:
        ok = (v.values or 0) == (p.values or 0) + off * WIDTH[vt]
    if p.validity is not None:
        ok = ok and off % 8 == 0 and v.validity == p.validity + off // 8
    return bool(ok)


def assert_view(view, copy=False):
    """every view-class case asserts this, the control arm the opposite: a slice that starts to copy must not turn the tests into no-ops"""
    got = is_view(view.parent, view, view.off)
    assert got == (not copy), f"slice at row {view.off} is {'a view' if got else 'a copy'}, expected {'a copy' if copy else 'a view'}"


@dataclass(frozen=True)
class ViewCase:
    id: str
    off: int
    n: int
    nulls: str = "none"          # none | some | all | clean (no NULL in the window, validity in the parent)
    off2: int = -1               # >= 0: a view of a view, off then off2
    tail: int = TAIL

    @property
    def nullable(self):
        return self.nulls != "none"

    def is_copy(self, boolean):
        """class E: a column with a bitmap (validity, or Boolean values) cannot be re-based at bit granularity"""
        return (self.nullable or boolean) and (self.off + max(self.off2, 0)) % 64 != 0

    def window(self, kind, rng):
        return rand_array(kind, self.n, {"none": 0.0, "clean": 0.0, "some": 0.2, "all": 1.0}[self.nulls], rng)

    def make(self, ctx, kind, rng, arr=None):
        """-> (view, expected) with the view-ness asserted; `arr`: the window (then `kind` may be None), else a random one of `kind`"""
        arr = self.window(kind, rng) if arr is None else arr
        assert len(arr) == self.n
        fv = self.nulls == "clean" or (self.nullable and arr.null_count == 0)
        if self.off2 >= 0:
            view, exp = view_of_view(ctx, arr, self.off, self.off2, fv)
        else:
            view, exp = as_view(ctx, arr, self.off, self.tail, True, fv)
        assert (view.parent.describe().validity is not None) == self.nullable
        assert_view(view, copy=self.is_copy(pa.types.is_boolean(arr.type)))
        return view, exp

    def host(self, kind, rng, arr=None):
        """-> (parent on the host, offset of the window, window): what `make` imports, without a device"""
        arr = self.window(kind, rng) if arr is None else arr
        fv = self.nulls == "clean" or (self.nullable and arr.null_count == 0)
        o = self.off + max(self.off2, 0)
        return parent_arrow(arr, o, self.tail, True, fv), o, arr


# classes A / B / D (by kind): non-null columns at any row offset
CLASS_A = [ViewCase(f"A-off{o}", o, 1000) for o in (1, 3, 64, 65)]
# class C: offset % 64 == 0, length % 64 in {0, 1, 63}
CLASS_C = [ViewCase(f"C-off{o}-n{n}", o, n, "some") for o in (64, 128) for n in (1024, 961, 1023)]
CLASS_C_EDGE = [ViewCase("C-no-null-in-window", 64, 961, "clean"), ViewCase("C-only-nulls", 128, 1023, "all")]
# class E: the control arm
CLASS_E = [ViewCase(f"E-off{o}", o, 1000, "some") for o in (1, 65)]
SPECIAL = [ViewCase("A-view-of-view", 1, 1000, "none", off2=2), ViewCase("C-view-of-view", 64, 961, "some", off2=64),
           ViewCase("A-zero-length-at-end", 77, 0, "none", tail=0), ViewCase("C-zero-length-at-end", 128, 0, "some", tail=0),
           ViewCase("A-whole-parent", 0, 1000, "none", tail=0), ViewCase("C-whole-parent", 0, 961, "some", tail=0)]
VIEW_CASES = CLASS_A + CLASS_C + CLASS_C_EDGE + CLASS_E + SPECIAL
# one of each class, for the operators whose cases are expensive
VIEW_CASES_SHORT = [CLASS_A[0], CLASS_A[3], CLASS_C[1], CLASS_C[5], CLASS_C_EDGE[0], CLASS_C_EDGE[1], CLASS_E[0], SPECIAL[0], SPECIAL[1], SPECIAL[3]]
