"""-m gpu: Timestamp columns on the device -- import / export, date_part and date_trunc (k_ts_part, k_ts_trunc), the casts, and every operator that takes
an Int64 column taking a Timestamp column.

Oracles.  date_part, date_trunc and the casts: tests/timestamp_reference.py (pinned to the reference's own answers by tests/test_timestamp_reference.py),
bit-exact in values and validity.  The operators: a Timestamp is an Int64 count since the epoch and hashes as one, so an operator over a Timestamp column must
give exactly what it gives over the same buffer typed Int64, with the Timestamp type on its output columns -- no tolerance, no second implementation."""
import datetime

import numpy as np
import pyarrow as pa
import pytest

import dfgpu
import timestamp_reference as ref
from dfgpu import capi
from dfgpu import physical_plan as ops
from test_gpu_expr import OPCODE, exported, same
from test_gpu_pagg import forced as forced_preaggregate
from test_gpu_pjoin import forced as forced_partitioned_join

pytestmark = pytest.mark.gpu

UNITS = list(ref.UNITS)
BLOCK = 256
# k_ts_part / k_ts_trunc take two instants per lane when both pointers are 16-byte aligned: no row, one (the odd tail alone), a pair, a pair and the tail; a
# validity word less a bit, exactly, a bit more; a workgroup of rows less one, exactly, one more; two workgroups less and more one
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2 * BLOCK - 1, 2 * BLOCK + 1]
EPOCH = datetime.date(1970, 1, 1).toordinal()
# second, minute, hour, day, week (Mondays), month, quarter and year boundaries on both sides of 1970; the leap days 1900 did not have and 2000 had; years whose
# ISO week 53 spills into January (2020/21, 2015/16, 2009/10, 1964/65) and a week 1 that starts in December (2024-12-30)
BOUNDARIES = ["1969-12-31T23:59:59", "1969-12-31T23:59:00", "1969-12-31T23:00:00", "1970-01-01T00:00:00", "1970-01-01T00:00:01", "1970-01-01T00:01:00", "1970-01-01T01:00:00",
              "1969-12-29T00:00:00", "1970-01-05T00:00:00", "1969-12-01T00:00:00", "1970-02-01T00:00:00", "1969-10-01T00:00:00", "1970-04-01T00:00:00", "1969-01-01T00:00:00",
              "1971-01-01T00:00:00", "1900-02-28T00:00:00", "1900-03-01T00:00:00", "2000-02-29T00:00:00", "2000-03-01T00:00:00", "2020-12-31T00:00:00", "2021-01-04T00:00:00",
              "2015-12-31T00:00:00", "2016-01-04T00:00:00", "2010-01-04T00:00:00", "1964-12-28T00:00:00", "1965-01-04T00:00:00", "2024-12-30T00:00:00", "2022-08-03T14:38:50"]


def named_values(unit, wide):
    """both edges of the nanosecond window and +-1 unit around every boundary; wide (date_part over s / ms / us): also the first and the last instant of the years 1..9999"""
    lo, hi = ref.window(unit)
    vals = [lo, lo + 1, hi - 1, hi]
    for b in BOUNDARIES:
        v = ref.from_iso(b, unit)
        vals += [v - 1, v, v + 1]
    if wide and unit != "ns":
        per_day = 86400 * ref.UNITS[unit]
        vals += [(1 - EPOCH) * per_day, (datetime.date.max.toordinal() - EPOCH + 1) * per_day - 1]
    return vals


def pool(unit, wide):
    """the value set in a fixed order: the named values first (shuffled among themselves, so that every prefix from 255 rows on holds all of them and the short
    prefixes differ from unit to unit), then random instants inside the window and, when wide, in the years 1..9999.  Every column of the tests below is a prefix
    of it, and one of them the whole of it."""
    lo, hi = ref.window(unit)
    rng = np.random.default_rng(len(unit) + 40)
    named = named_values(unit, wide)
    rng.shuffle(named)
    vals = named + [int(x) for x in rng.integers(lo, hi, 500, dtype=np.int64)]
    if wide and unit != "ns":
        first, last = named_values(unit, True)[-2:]
        vals += [int(x) for x in rng.integers(first, last, 300, dtype=np.int64)]
    return [int(v) for v in vals]


def ts_array(values, unit):
    return pa.array(values, type=pa.timestamp(unit))


def utf8(s):
    return pa.array([s], type=pa.utf8())


def call(ctx, fn, name, col, col_scalar=False):
    return ctx.scalar_function(fn, [ctx.from_arrow(utf8(name)), col], [True, col_scalar])


def offset_view(ctx, values, unit, offset=1):
    """rows [offset, offset + n) of a parent without NULLs: a view (include/dfgpu.h) whose base is 8-byte but, at an odd offset of a fresh allocation, not 16-byte aligned"""
    parent = ctx.from_arrow(ts_array([values[0] if values else 0] * offset + values + [0, 0, 0], unit))
    v = parent.slice(offset, len(values))
    assert v.describe().values == parent.describe().values + 8 * offset
    return v


# ------------------------------------------------------------------------------------------------ import / export
def check_round_trip_and_type_codes(ctx, unit):
    vals = pool(unit, False)[:100]
    for arr in (ts_array(vals, unit), ts_array([None if i % 3 == 0 else v for i, v in enumerate(vals)], unit), ts_array([], unit), ts_array([None], unit)):
        d = ctx.from_arrow(arr)
        assert d.type == ref.TYPE_CODE[unit] and d.describe().type == ref.TYPE_CODE[unit]
        assert same(d.to_arrow(), arr)
    dic = pa.DictionaryArray.from_arrays(pa.array([2, 0, None, 1, 2, 2], type=pa.int32()), ts_array([vals[0], None, vals[2]], unit))
    d = ctx.from_arrow(dic)
    assert d.type == capi.DICTIONARY and d.describe().dictionary.contents.type == ref.TYPE_CODE[unit]
    back = d.to_arrow()
    assert back.type == dic.type and back.to_pylist() == dic.to_pylist()
    with pytest.raises(dfgpu.DfgpuError) as e:          # a time zone stays outside the device
        ctx.from_arrow(pa.array(vals[:3], type=pa.timestamp(unit, tz="UTC")))
    assert e.value.status == 4 and "unsupported Arrow format" in str(e.value)
    import torch
    t = torch.tensor(vals[:7], dtype=torch.int64, device="cuda")
    w = ctx.wrap_tensor(t, ref.TYPE_CODE[unit])
    assert w.type == ref.TYPE_CODE[unit] and same(w.to_arrow(), ts_array(vals[:7], unit))
    s = ctx.concat([d2 := ctx.from_arrow(ts_array(vals[:5], unit)), d2.slice(1, 3)])
    assert same(s.to_arrow(), ts_array(vals[:5] + vals[1:4], unit))


# ------------------------------------------------------------------------------------------------ date_part / date_trunc, bit-exact
def reference_column(fn, name, unit, values):
    """(rows the reference defines, their results): a row outside date_trunc's window is left to check_date_trunc_errors"""
    keep, want = [], []
    for v in values:
        try:
            want.append(ref.date_part_ts(name, v, unit) if fn == ref.FN_DATE_PART else ref.date_trunc(name, v, unit))
            keep.append(v)
        except ref.OutOfRange:
            pass
    return keep, want


def typed_result(fn, unit, want):
    return pa.array(want, type=pa.float64()) if fn == ref.FN_DATE_PART else ts_array(want, unit)


def check_every_name_every_length_aligned_and_not(ctx, fn, unit):
    names = ref.PARTS if fn == ref.FN_DATE_PART else ref.GRANULARITIES
    values = pool(unit, fn == ref.FN_DATE_PART)
    named = set(named_values(unit, fn == ref.FN_DATE_PART))
    assert len(values) >= max(LENGTHS) and named <= set(values[:255])
    for k, name in enumerate(names):
        keep, want = reference_column(fn, name, unit, values)          # computed once per name, shared by every length
        assert len(keep) >= len(values) - 8 and len(named - set(keep)) <= 8          # date_trunc: only the few rows next to the window's lower edge are left to the error test
        spelled = name.upper() if k % 2 else name
        for n in LENGTHS + [len(keep)]:                                # the last one: the whole value set
            expect = typed_result(fn, unit, want[:n])
            got = call(ctx, fn, spelled, ctx.from_arrow(ts_array(keep[:n], unit)))
            assert same(exported(ctx, got), expect), (name, unit, n)
            if n:
                got = call(ctx, fn, spelled, offset_view(ctx, keep[:n], unit))
                assert same(exported(ctx, got), expect), (name, unit, n, "view")


def check_validity_scalar_and_dictionary(ctx, fn, unit):
    names = ref.PARTS if fn == ref.FN_DATE_PART else ref.GRANULARITIES
    values = pool(unit, fn == ref.FN_DATE_PART)
    for name in names:
        keep, want = reference_column(fn, name, unit, values)
        n = len(keep)                                                  # the whole value set; every fifth row NULL, and in a second pass its neighbours instead
        for shift in (1, 2):
            nulls = [i % 5 == shift for i in range(n)]
            col = [None if z else v for v, z in zip(keep, nulls)]
            expect = typed_result(fn, unit, [None if z else w for w, z in zip(want, nulls)])
            assert same(exported(ctx, call(ctx, fn, name, ctx.from_arrow(ts_array(col, unit)))), expect), (name, "validity", shift)
        # a scalar instant, and a NULL one
        got = call(ctx, fn, name, ctx.from_arrow(ts_array([keep[3]], unit)), col_scalar=True)
        assert same(exported(ctx, got), typed_result(fn, unit, [want[3]])), (name, "scalar")
        got = call(ctx, fn, name, ctx.from_arrow(ts_array([None], unit)), col_scalar=True)
        assert same(exported(ctx, got), typed_result(fn, unit, [None])), (name, "NULL scalar")
        # a dictionary smaller than the column, with a NULL entry and NULL codes (date_part: once per entry; date_trunc: decoded first)
        entries = keep[:16] + [None]
        codes = [None if i % 11 == 4 else (i * 7) % 17 for i in range(300)]
        dic = pa.DictionaryArray.from_arrays(pa.array(codes, type=pa.int16()), ts_array(entries, unit))
        w_entries = want[:16] + [None]
        expect = typed_result(fn, unit, [None if c is None else w_entries[c] for c in codes])
        assert same(exported(ctx, call(ctx, fn, name, ctx.from_arrow(dic))), expect), (name, "dictionary")
    # a NULL part name gives NULL rows (date_part.rs answers an error for it only at planning; the device keeps the Date32 behaviour)
    if fn == ref.FN_DATE_PART:
        got = ctx.scalar_function(fn, [ctx.from_arrow(pa.array([None], type=pa.utf8())), ctx.from_arrow(ts_array(values[:5], unit))], [True, False])
        assert got.to_arrow().null_count == 5


def check_years_outside_1_to_9999_do_not_fault(ctx):
    """unpinned values, as for Date32: the call returns and every row is a finite number"""
    extremes = [-2**63, -2**63 + 1, -2**62, 2**62, 2**63 - 1]
    for unit in ("s", "ms", "us"):
        for part in ref.PARTS:
            out = call(ctx, ref.FN_DATE_PART, part, ctx.from_arrow(ts_array(extremes * 13, unit))).to_arrow()
            assert len(out) == 65 and out.null_count == 0 and np.all(np.isfinite(np.asarray(out)))


# ------------------------------------------------------------------------------------------------ date_trunc errors
def status_of(fn):
    with pytest.raises(dfgpu.DfgpuError) as e:
        fn()
    return e.value.status, str(e.value)


def check_date_trunc_errors(ctx, unit):
    lo, hi = ref.window(unit)
    good = pool(unit, False)[:100]
    good = [v for v in good if lo + 400 * 86400 * ref.UNITS[unit] < v]
    col = ctx.from_arrow(ts_array(good, unit))
    st, msg = status_of(lambda: call(ctx, ref.FN_DATE_TRUNC, "fortnight", col))
    assert st == 1 and "Unsupported date_trunc granularity: fortnight" in msg
    for bad_name in (pa.array([None], type=pa.utf8()),):
        st, msg = status_of(lambda: ctx.scalar_function(ref.FN_DATE_TRUNC, [ctx.from_arrow(bad_name), col], [True, False]))
        assert st == 1 and "Granularity of `date_trunc` must be non-null scalar Utf8" in msg
    per_row = ctx.from_arrow(pa.array(["day"] * len(good), type=pa.utf8()))
    st, msg = status_of(lambda: ctx.scalar_function(ref.FN_DATE_TRUNC, [per_row, col], [False, False]))
    assert st == 1 and "Granularity of `date_trunc` must be non-null scalar Utf8" in msg
    st, _ = status_of(lambda: ctx.scalar_function(ref.FN_DATE_TRUNC, [ctx.from_arrow(utf8("day")), col, col], [True, False, False]))
    assert st == 4                                                        # exactly two arguments
    st, _ = status_of(lambda: call(ctx, ref.FN_DATE_TRUNC, "day", ctx.from_arrow(pa.array(good, type=pa.int64()))))
    assert st == 4                                                        # Int64 is no Timestamp: the planner coerces first
    # a row outside the window: the lower edge truncated to its day lies below it in every unit; beyond the window in the coarser units
    outside = [(lo, "day")] + ([(lo - 1, "second"), (hi + 1, "microsecond"), (2**63 - 1, "year")] if unit != "ns" else [])
    for v, gran in outside:
        with pytest.raises(ref.OutOfRange):
            ref.date_trunc(gran, v, unit)
        rows = good[:70] + [v] + good[70:75]
        at = 70
        st, msg = status_of(lambda: call(ctx, ref.FN_DATE_TRUNC, gran, ctx.from_arrow(ts_array(rows, unit))))
        assert st == 1 and f"Timestamp {v} out of range" in msg, (v, gran, msg)
        st, msg = status_of(lambda: call(ctx, ref.FN_DATE_TRUNC, gran, offset_view(ctx, rows, unit)))
        assert st == 1 and "out of range" in msg
        # silent when the row is NULL ...
        nullable = [None if i == at else r for i, r in enumerate(rows)]
        want = [None if r is None else ref.date_trunc(gran, r, unit) for r in nullable]
        assert same(call(ctx, ref.FN_DATE_TRUNC, gran, ctx.from_arrow(ts_array(nullable, unit))).to_arrow(), ts_array(want, unit))
        # ... or deselected (its value is then unspecified and stays behind the selection)
        sel = [i != at for i in range(len(rows))]
        ctx.push_row_selection(ctx.from_arrow(pa.array(sel)))
        try:
            got = retyped(call(ctx, ref.FN_DATE_TRUNC, gran, ctx.from_arrow(ts_array(rows, unit))), unit).to_pylist()
        finally:
            ctx.pop_row_selection()
        assert [g for g, s in zip(got, sel) if s] == [ref.date_trunc(gran, r, unit) for r, s in zip(rows, sel) if s]
        # and raises again once selected
        st, _ = status_of(lambda: call(ctx, ref.FN_DATE_TRUNC, gran, ctx.from_arrow(ts_array(rows, unit))))
        assert st == 1


def check_date_trunc_inside_an_untaken_case_branch(ctx, task_ctx):
    unit = "s"
    lo, _ = ref.window(unit)
    vals = [0, 86399, lo, 86400 * 365, lo, -1]
    flags = [v != lo for v in vals]
    batch = ops.batch_from_arrow(ctx, pa.table({"t": ts_array(vals, unit), "ok": pa.array(flags)}))
    src = lambda: ops.MemoryExec([[batch]], batch.schema)
    trunc = lambda: ops.date_trunc(ops.Literal("day", pa.utf8()), ops.Column("t", 0))
    case = ops.CaseExpr(None, [(ops.Column("ok", 1), trunc())], None)
    got = pa.concat_tables([b.to_arrow() for b in ops.collect(ops.ProjectionExec([(case, "d")], src()), task_ctx)]).column(0).combine_chunks()
    assert same(got, ts_array([ref.date_trunc("day", v, unit) if f else None for v, f in zip(vals, flags)], unit))
    with pytest.raises(dfgpu.DfgpuError) as e:
        ops.collect(ops.ProjectionExec([(trunc(), "d")], src()), task_ctx)
    assert e.value.status == 1 and "out of range" in str(e.value)


# ------------------------------------------------------------------------------------------------ casts
def dev_cast(ctx, arr, to):
    return ctx.cast(ctx.from_arrow(arr), to).to_arrow()


def check_casts(ctx):
    rng = np.random.default_rng(3)
    for unit in UNITS:
        code = ref.TYPE_CODE[unit]
        ints = [None, -2**63, 2**63 - 1, -1, 0, 1] + [int(x) for x in rng.integers(-2**62, 2**62, 70, dtype=np.int64)]
        # Int64 <-> Timestamp: the values unchanged, the buffer shared
        i64 = ctx.from_arrow(pa.array(ints, type=pa.int64()))
        t = ctx.cast(i64, code)
        assert same(t.to_arrow(), ts_array(ints, unit)) and t.describe().values == i64.describe().values
        back = ctx.cast(t, capi.INT64)
        assert same(back.to_arrow(), pa.array(ints, type=pa.int64())) and back.describe().values == i64.describe().values
        dic = pa.DictionaryArray.from_arrays(pa.array([1, None, 0, 2], type=pa.int8()), pa.array([5, -7, None], type=pa.int64()))
        assert same(dev_cast(ctx, dic, code), ts_array([-7, None, 5, None], unit))
        for other in UNITS:
            f, t_ = ref.UNITS[unit], ref.UNITS[other]
            if t_ > f:          # finer: a checked multiply
                fit = (2**63 - 1) // (t_ // f)
                vals = [None, -fit, fit, -1, 0, 1] + [int(x) for x in rng.integers(-fit, fit, 70, dtype=np.int64)]
                assert same(dev_cast(ctx, ts_array(vals, unit), ref.TYPE_CODE[other]), ts_array([ref.cast_timestamp(v, unit, other) for v in vals], other))
                for bad in (fit + 1, -fit - 2):
                    with pytest.raises(ref.Overflow):
                        ref.cast_timestamp(bad, unit, other)
                    st, msg = status_of(lambda: dev_cast(ctx, ts_array(vals + [bad], unit), ref.TYPE_CODE[other]))
                    assert st == 1 and "overflow" in msg.lower()
                nul = pa.array([fit + 1, 5], type=pa.int64()).cast(pa.timestamp(unit))          # the overflowing row is NULL: silent
                nul = pa.Array.from_buffers(pa.timestamp(unit), 2, [pa.py_buffer(bytes([0b10])), nul.buffers()[1]])
                assert dev_cast(ctx, nul, ref.TYPE_CODE[other]).to_pylist()[0] is None
            elif t_ < f:        # coarser: toward zero.  Pre-epoch values only where truncation and floor agree (exact multiples); positive values anywhere
                d = f // t_
                vals = [None, 0, 1, d - 1, d, d + 1] + [int(x) for x in rng.integers(0, 2**62, 40, dtype=np.int64)] + [-int(x) * d for x in rng.integers(0, 2**62 // d, 40, dtype=np.int64)]
                assert same(dev_cast(ctx, ts_array(vals, unit), ref.TYPE_CODE[other]), ts_array([ref.cast_timestamp(v, unit, other) for v in vals], other))
        # Date32 <-> Timestamp
        per_day = 86400 * ref.UNITS[unit]
        top = min(2**31 - 1, (2**63 - 1) // per_day)
        days = [None, -top, top, -1, 0, 1, 18262, -25567]
        d32 = pa.array(days, type=pa.int32()).cast(pa.date32())
        assert same(dev_cast(ctx, d32, code), ts_array([ref.date32_to_timestamp(d, unit) for d in days], unit))
        if top < 2**31 - 1:
            st, msg = status_of(lambda: dev_cast(ctx, pa.array([0, top + 1], type=pa.int32()).cast(pa.date32()), code))
            assert st == 1 and "overflow" in msg.lower()
        vals = [None, 0, 1, per_day - 1, per_day, 2**63 - 1] + [int(x) for x in rng.integers(0, 2**62, 40, dtype=np.int64)] + [-int(x) * per_day for x in rng.integers(0, 2**62 // per_day, 40, dtype=np.int64)]
        want = pa.array([ref.timestamp_to_date32(v, unit) for v in vals], type=pa.int32()).cast(pa.date32())
        assert same(dev_cast(ctx, ts_array(vals, unit), capi.DATE32), want)
        # Utf8 <-> Timestamp and the other numeric types stay unimplemented
        for to in (capi.UTF8, capi.INT32, capi.FLOAT64, capi.DECIMAL128):
            st, _ = status_of(lambda: ctx.cast(ctx.from_arrow(ts_array([1], unit)), to, 10, 0))
            assert st == 4
        st, _ = status_of(lambda: dev_cast(ctx, pa.array(["2020-01-01"]), code))
        assert st == 4


# ------------------------------------------------------------------------------------------------ the Int64-equality oracle
def pair(ctx, ints, unit):
    """the same values as a Timestamp column and as an Int64 column"""
    a = pa.array(ints, type=pa.int64())
    return ctx.from_arrow(a.cast(pa.timestamp(unit))), ctx.from_arrow(a)


def retyped(out, unit):
    """a Timestamp result as the Int64 column it must equal; asserts the type on the way"""
    a = out.to_arrow() if hasattr(out, "to_arrow") else out
    assert a.type == pa.timestamp(unit), a.type
    return a.cast(pa.int64())


def keys_with_nulls(n, seed, card=40, null_frac=0.15):
    rng = np.random.default_rng(seed)
    k = rng.integers(-card, card, n) * 86_400_000_007
    return [None if z else int(v) for v, z in zip(k, rng.random(n) < null_frac)]


def check_compare_in_list_is_null_case(ctx, unit):
    n = 1000
    l, r = keys_with_nulls(n, 1), keys_with_nulls(n, 2)
    lt, li = pair(ctx, l, unit)
    rt, ri = pair(ctx, r, unit)
    st, si = pair(ctx, [l[5] if l[5] is not None else 7], unit)
    nt, ni = pair(ctx, [v if v is not None else 3 for v in l], unit)          # no NULLs: the scalar compare's fast path
    for op in ("=", "!=", "<", "<=", ">", ">=", "IS DISTINCT FROM", "IS NOT DISTINCT FROM"):
        assert same(exported(ctx, ctx.binary(OPCODE[op], lt, rt)), ctx.binary(OPCODE[op], li, ri).to_arrow()), op
        assert same(exported(ctx, ctx.binary(OPCODE[op], lt, st, False, True)), ctx.binary(OPCODE[op], li, si, False, True).to_arrow()), op
        assert same(exported(ctx, ctx.binary(OPCODE[op], st, nt, True, False)), ctx.binary(OPCODE[op], si, ni, True, False).to_arrow()), op
    ctx.profile_select(None); ctx.profile_enable(True); ctx.profile_read()
    ctx.binary(OPCODE["<"], nt, st, False, True)
    kernels = set(ctx.profile_read()); ctx.profile_enable(False)
    assert "k_compare_scalar_fast" in kernels          # column / scalar without NULLs keeps the Int64 fast path
    other = "ms" if unit == "s" else "s"
    status, msg = status_of(lambda: ctx.binary(OPCODE["="], lt, ctx.from_arrow(ts_array(l, other))))          # two units are two types
    assert status == 4 and "the planner coerces first" in msg
    for op in "+-":
        status, _ = status_of(lambda: ctx.binary(OPCODE[op], lt, rt))
        assert status == 4                                 # no arithmetic on timestamps
    lst_t, lst_i = pair(ctx, [l[1], None, r[2], 12345], unit)
    for neg in (False, True):
        assert same(exported(ctx, ctx.in_list(lt, lst_t, neg)), ctx.in_list(li, lst_i, neg).to_arrow())
    assert same(exported(ctx, ctx.is_null(lt)), ctx.is_null(li).to_arrow()) and same(exported(ctx, ctx.is_null(lt, True)), ctx.is_null(li, True).to_arrow())
    w1 = ctx.binary(OPCODE["<"], li, ri)
    w2 = ctx.binary(OPCODE[">"], li, si, False, True)
    got = ctx.case([w1, w2], [lt, st], rt, [False, True])
    assert same(retyped(got, unit), ctx.case([w1, w2], [li, si], ri, [False, True]).to_arrow())
    got = ctx.case([w1], [None], lt)
    assert same(retyped(got, unit), ctx.case([w1], [None], li).to_arrow())


def check_take_filter_concat_slice_sort(ctx, unit):
    n = 1500
    k = keys_with_nulls(n, 3, card=300)
    t, i = pair(ctx, k, unit)
    idx = ctx.from_arrow(pa.array([None if j % 17 == 0 else (j * 7919) % n for j in range(700)], type=pa.uint32()))
    assert same(retyped(ctx.take(t, idx), unit), ctx.take(i, idx).to_arrow())
    mask = ctx.from_arrow(pa.array([None if j % 13 == 0 else j % 3 != 0 for j in range(n)]))
    assert same(retyped(ctx.filter(t, mask), unit), ctx.filter(i, mask).to_arrow())
    assert same(retyped(ctx.concat([t, t.slice(64, 100), t.slice(5, 9)]), unit), ctx.concat([i, i.slice(64, 100), i.slice(5, 9)]).to_arrow())
    payload = ctx.from_arrow(pa.array(np.arange(n, dtype=np.int64)))
    for desc in (False, True):
        for nulls_first in (False, True):
            a = ctx.sort_to_indices([t], [desc], [nulls_first])
            b = ctx.sort_to_indices([i], [desc], [nulls_first])
            assert np.array_equal(a.to_numpy(), b.to_numpy())
            assert same(retyped(ctx.take(t, a), unit), ctx.take(i, b).to_arrow())          # as the sorted key
            # as a payload of another key, and as the second key behind it
            few = ctx.from_arrow(pa.array([j % 5 for j in range(n)], type=pa.int32()))
            a2, b2 = ctx.sort_to_indices([few, t], [False, desc], [True, nulls_first]), ctx.sort_to_indices([few, i], [False, desc], [True, nulls_first])
            assert np.array_equal(a2.to_numpy(), b2.to_numpy())
            assert same(retyped(ctx.take(t, a2), unit), ctx.take(i, b2).to_arrow()) and np.array_equal(ctx.take(payload, a2).to_numpy(), ctx.take(payload, b2).to_numpy())
    a, b = ctx.sort_to_indices([t], [False], [True], fetch=10), ctx.sort_to_indices([i], [False], [True], fetch=10)
    assert np.array_equal(a.to_numpy(), b.to_numpy())


def check_group_by_and_accumulators(ctx, unit):
    n = 3000
    k = keys_with_nulls(n, 4)
    v = keys_with_nulls(n, 5, card=1000)
    kt, ki = pair(ctx, k, unit)
    vt, vi = pair(ctx, v, unit)
    gt, gi = dfgpu.GroupValues(ctx, 1), dfgpu.GroupValues(ctx, 1)
    ids_t, ids_i = gt.intern([kt]), gi.intern([ki])
    ng = len(gt)
    assert np.array_equal(ids_t.to_numpy(), ids_i.to_numpy()) and ng == len(gi) > 1
    assert same(retyped(gt.emit()[0], unit), gi.emit()[0].to_arrow())
    # without NULLs: the primitive-key table; clustered: run numbers
    for keys in ([x if x is not None else 0 for x in k], sorted(x if x is not None else 0 for x in k)):
        pt, pi = pair(ctx, keys, unit)
        g1, g2 = dfgpu.GroupValues(ctx, 1), dfgpu.GroupValues(ctx, 1)
        assert np.array_equal(g1.intern([pt]).to_numpy(), g2.intern([pi]).to_numpy())
        assert same(retyped(g1.emit()[0], unit), g2.emit()[0].to_arrow())
    code = ref.TYPE_CODE[unit]
    for kind in (capi.AGG_MIN, capi.AGG_MAX):
        at, ai = dfgpu.GroupsAccumulator(ctx, kind, code), dfgpu.GroupsAccumulator(ctx, kind, capi.INT64)
        at.update_batch(vt, ids_t, None, ng); ai.update_batch(vi, ids_i, None, ng)
        st_t, st_i = at.state(), ai.state()
        assert same(retyped(st_t[0], unit), st_i[0].to_arrow())
        mt, mi = dfgpu.GroupsAccumulator(ctx, kind, code), dfgpu.GroupsAccumulator(ctx, kind, capi.INT64)
        gid = ctx.from_arrow(pa.array(np.arange(ng, dtype=np.uint32)))
        mt.merge_batch(st_t, gid, None, ng); mi.merge_batch(st_i, gid, None, ng)
        assert same(retyped(mt.evaluate(), unit), mi.evaluate().to_arrow())
        et, ei = dfgpu.GroupsAccumulator(ctx, kind, code), dfgpu.GroupsAccumulator(ctx, kind, capi.INT64)
        et.update_batch(vt, ids_t, None, ng); ei.update_batch(vi, ids_i, None, ng)
        assert same(retyped(et.evaluate(), unit), ei.evaluate().to_arrow())
    ct, ci = dfgpu.GroupsAccumulator(ctx, capi.AGG_COUNT, code), dfgpu.GroupsAccumulator(ctx, capi.AGG_COUNT, capi.INT64)
    ct.update_batch(vt, ids_t, None, ng); ci.update_batch(vi, ids_i, None, ng)
    assert same(ct.evaluate().to_arrow(), ci.evaluate().to_arrow())
    for kind in (capi.AGG_SUM, capi.AGG_AVG):          # refused, as in the reference
        with pytest.raises(dfgpu.DfgpuError):
            dfgpu.GroupsAccumulator(ctx, kind, code)
    # dfgpu_agg_preaggregate: one key column without NULLs
    dense = [x if x is not None else 11 for x in k]
    pt, pi = pair(ctx, dense, unit)
    with forced_preaggregate(ctx):
        keys_t, states_t = dfgpu.agg_preaggregate(ctx, pt, [capi.AGG_COUNT, capi.AGG_MIN, capi.AGG_MAX], [None, vt, vt])
        keys_i, states_i = dfgpu.agg_preaggregate(ctx, pi, [capi.AGG_COUNT, capi.AGG_MIN, capi.AGG_MAX], [None, vi, vi])
    assert same(retyped(keys_t, unit), keys_i.to_arrow())
    assert same(states_t[0][0].to_arrow(), states_i[0][0].to_arrow())
    for j in (1, 2):
        assert same(retyped(states_t[j][0], unit), states_i[j][0].to_arrow())


def check_count_distinct_through_a_plan(ctx, task_ctx):
    unit, n = "ms", 2000
    g = [j % 7 for j in range(n)]
    v = keys_with_nulls(n, 6, card=25)
    out = {}
    for name, typ in (("t", pa.timestamp(unit)), ("i", pa.int64())):
        batch = ops.batch_from_arrow(ctx, pa.table({"g": pa.array(g, type=pa.int32()), "v": pa.array(v, type=pa.int64()).cast(typ)}))
        field = ops.Field("v", ref.TYPE_CODE[unit] if name == "t" else capi.INT64)
        partial = ops.AggregateExec("Partial", [(ops.Column("g", 0), "g")], [ops.AggregateFunctionExpr("COUNT DISTINCT", ops.Column("v", 1), "d", input_field=field)],
                                    ops.MemoryExec([[batch]], batch.schema))
        final = ops.AggregateExec("Final", [(ops.Column("g", 0), "g")], [ops.AggregateFunctionExpr("COUNT DISTINCT", ops.Column("d", 1), "d", input_field=field)], partial)
        t = pa.concat_tables([b.to_arrow() for b in ops.collect(final, task_ctx)])
        out[name] = dict(zip(t.column(0).to_pylist(), t.column(1).to_pylist()))
    want = {k: len({x for x, gg in zip(v, g) if gg == k and x is not None}) for k in range(7)}
    assert out["t"] == out["i"] == want


def check_join_keys_and_partitioning(ctx, unit):
    nb, npr = 1200, 4000
    b = keys_with_nulls(nb, 7, card=400)
    p = keys_with_nulls(npr, 8, card=500)
    bt, bi = pair(ctx, b, unit)
    pt, pi = pair(ctx, p, unit)
    for nen in (False, True):          # the global table
        x, y = dfgpu.JoinTable(ctx, [bt], null_equals_null=nen).probe([pt]), dfgpu.JoinTable(ctx, [bi], null_equals_null=nen).probe([pi])
        assert np.array_equal(x[0].to_numpy(), y[0].to_numpy()) and np.array_equal(x[1].to_numpy(), y[1].to_numpy()) and len(x[0]) > 0
    # unique keys without NULLs: the rank index / bitmap paths, then the partitioned table
    ub = sorted({v for v in b if v is not None})
    up = [v if v is not None else 1 for v in p]
    ubt, ubi = pair(ctx, ub, unit)
    upt, upi = pair(ctx, up, unit)
    x, y = dfgpu.JoinTable(ctx, [ubt]).probe([upt]), dfgpu.JoinTable(ctx, [ubi]).probe([upi])
    assert np.array_equal(x[0].to_numpy(), y[0].to_numpy()) and np.array_equal(x[1].to_numpy(), y[1].to_numpy()) and len(x[0]) > 0
    # the probe with the scan filter folded in: the predicate column and its literal are Timestamps too
    # (a sorted unique build over a dense domain: the table that keeps a membership bitmap)
    rng = np.random.default_rng(12)
    dense_b = sorted({int(v) for v in rng.integers(1000, 5000, 1500)})
    dense_p = [int(v) for v in rng.integers(0, 6000, npr)]
    dbt, dbi = pair(ctx, dense_b, unit)
    dpt, dpi = pair(ctx, dense_p, unit)
    lit_t, lit_i = pair(ctx, [3000], unit)
    plain = dfgpu.JoinTable(ctx, [dbt]).probe([dpt])
    fx = dfgpu.JoinTable(ctx, [dbt]).probe_fused([dpt], dpt, OPCODE[">="], lit_t)
    fy = dfgpu.JoinTable(ctx, [dbi]).probe_fused([dpi], dpi, OPCODE[">="], lit_i)
    assert fx is not None and fy is not None          # the Timestamp table takes the fused form where the Int64 table does
    assert np.array_equal(fx[0].to_numpy(), fy[0].to_numpy()) and np.array_equal(fx[1].to_numpy(), fy[1].to_numpy()) and 0 < len(fx[1]) < len(plain[1])
    with forced_partitioned_join(ctx, rows_per_partition=256) as f:
        x, y = dfgpu.JoinTable(ctx, [bt]).probe([pt]), dfgpu.JoinTable(ctx, [bi]).probe([pi])
        kernels = f.kernels()
    assert np.array_equal(x[0].to_numpy(), y[0].to_numpy()) and np.array_equal(x[1].to_numpy(), y[1].to_numpy())
    assert any(k.startswith("k_pj") or "pj_" in k for k in kernels), kernels
    # hash repartition into 8, and the columns moved with it
    ht, hi = ctx.hash_columns([pt]), ctx.hash_columns([pi])
    assert np.array_equal(ht.to_numpy(), hi.to_numpy())
    (rt, ct), (ri, ci) = ctx.hash_partition([pt], 8), ctx.hash_partition([pi], 8)
    assert ct == ci and np.array_equal(rt.to_numpy(), ri.to_numpy())
    mt, mi = ctx.partition_columns([pt], 8, [pt, upt]), ctx.partition_columns([pi], 8, [pi, upi])
    assert mt[2] == mi[2] and np.array_equal(mt[1].to_numpy(), mi[1].to_numpy())
    for a, bb in zip(mt[0], mi[0]):
        assert (a is None) == (bb is None)
        if a is not None:
            assert same(retyped(a, unit), bb.to_arrow())


def check_sort_merge_join_key(ctx, task_ctx):
    unit = "us"
    l = sorted(v for v in keys_with_nulls(600, 9, card=80) if v is not None)
    r = sorted(v for v in keys_with_nulls(700, 10, card=90) if v is not None)
    tables = {}
    for name, typ in (("t", pa.timestamp(unit)), ("i", pa.int64())):
        lb = ops.batch_from_arrow(ctx, pa.table({"k": pa.array(l, type=pa.int64()).cast(typ), "a": pa.array(range(len(l)), type=pa.int64())}))
        rb = ops.batch_from_arrow(ctx, pa.table({"k2": pa.array(r, type=pa.int64()).cast(typ), "b": pa.array(range(len(r)), type=pa.int64())}))
        plan = ops.SortMergeJoinExec(ops.MemoryExec([[lb]], lb.schema), ops.MemoryExec([[rb]], rb.schema), [(ops.Column("k", 0), ops.Column("k2", 0))], "Full")
        tables[name] = pa.concat_tables([b.to_arrow() for b in ops.collect(plan, task_ctx)])
    t, i = tables["t"], tables["i"]
    assert t.num_rows == i.num_rows > 0 and t.column(0).type == pa.timestamp(unit) and t.column(2).type == pa.timestamp(unit)
    for c in range(4):
        assert t.column(c).cast(pa.int64()).equals(i.column(c)), c


# ------------------------------------------------------------------------------------------------ ClickBench-shaped plans
def event_times(n=5000):
    rng = np.random.default_rng(43)
    base = ref.from_iso("2013-07-14T20:00:00", "s")
    return [int(x) for x in base + rng.integers(0, 3 * 3600, n)]


def check_q43_shaped_plan(ctx, task_ctx):
    """Filter (time range) -> Projection date_trunc('minute', to_timestamp_seconds(EventTime)) -> Aggregate COUNT(*) -> Sort"""
    ev = event_times()
    lo, hi = ref.from_iso("2013-07-14T20:30:00", "s"), ref.from_iso("2013-07-14T22:10:30", "s")
    batch = ops.batch_from_arrow(ctx, pa.table({"EventTime": pa.array(ev, type=pa.int64())}))
    ts = lambda: ops.to_timestamp_seconds(ops.Column("EventTime", 0))
    lit = lambda v: ops.Literal(v, pa.timestamp("s"))
    f = ops.FilterExec(ops.BinaryExpr(ops.BinaryExpr(ts(), ">=", lit(lo)), "AND", ops.BinaryExpr(ts(), "<", lit(hi))), ops.MemoryExec([[batch]], batch.schema))
    proj = ops.ProjectionExec([(ops.date_trunc(ops.Literal("minute", pa.utf8()), ts()), "M")], f)
    agg = ops.AggregateExec("Single", [(ops.Column("M", 0), "M")], [ops.AggregateFunctionExpr("COUNT", None, "PageViews")], proj)
    plan = ops.SortExec([ops.PhysicalSortExpr(ops.Column("M", 0))], agg)
    out = pa.concat_tables([b.to_arrow() for b in ops.collect(plan, task_ctx)])
    want = {}
    for e in ev:
        if lo <= e < hi:
            m = ref.date_trunc("minute", e, "s")
            want[m] = want.get(m, 0) + 1
    assert out.column(0).type == pa.timestamp("s")
    assert out.column(0).cast(pa.int64()).to_pylist() == sorted(want) and out.column(1).to_pylist() == [want[m] for m in sorted(want)] and len(want) > 90


def check_q19_shaped_plan(ctx, task_ctx):
    """extract(minute FROM to_timestamp_seconds(EventTime)) as the group key"""
    ev = event_times()
    batch = ops.batch_from_arrow(ctx, pa.table({"EventTime": pa.array(ev, type=pa.int64())}))
    key = ops.date_part(ops.Literal("minute", pa.utf8()), ops.to_timestamp_seconds(ops.Column("EventTime", 0)))
    proj = ops.ProjectionExec([(key, "m")], ops.MemoryExec([[batch]], batch.schema))
    agg = ops.AggregateExec("Single", [(ops.Column("m", 0), "m")], [ops.AggregateFunctionExpr("COUNT", None, "c")], proj)
    plan = ops.SortExec([ops.PhysicalSortExpr(ops.Column("m", 0))], agg)
    out = pa.concat_tables([b.to_arrow() for b in ops.collect(plan, task_ctx)])
    want = {}
    for e in ev:
        m = ref.date_part_ts("minute", e, "s")
        want[m] = want.get(m, 0) + 1
    assert out.column(0).type == pa.float64() and out.column(0).to_pylist() == sorted(want) and out.column(1).to_pylist() == [want[m] for m in sorted(want)] and len(want) == 60


# ------------------------------------------------------------------------------------------------ the tests
# One collected test per area; inside, every unit / function / operator is a case of its own: a failing case does not stop the cases after it, and the test's
# failure names all of them.
def run_cases(cases):
    failed = []
    for label, fn in cases:
        try:
            fn()
        except Exception as e:          # an assertion, or an error status of the library where none was expected
            failed.append(f"{label}: {type(e).__name__}: {e}")
    assert not failed, "\n".join([f"{len(failed)} of {len(cases)} cases failed"] + failed)


def test_import_export_wrap_and_views(ctx):
    run_cases([(unit, lambda unit=unit: check_round_trip_and_type_codes(ctx, unit)) for unit in UNITS])


def bit_exact_cases(ctx, fn):
    return [(f"{what.__name__}[{unit}]", lambda what=what, unit=unit: what(ctx, fn, unit)) for unit in UNITS
            for what in (check_every_name_every_length_aligned_and_not, check_validity_scalar_and_dictionary)]


def test_date_part_bit_exact(ctx):
    run_cases(bit_exact_cases(ctx, ref.FN_DATE_PART) + [("years outside 1..9999", lambda: check_years_outside_1_to_9999_do_not_fault(ctx))])


def test_date_trunc_bit_exact(ctx):
    run_cases(bit_exact_cases(ctx, ref.FN_DATE_TRUNC))


def test_date_trunc_errors_selection_and_case(ctx, task_ctx):
    run_cases([(f"errors[{unit}]", lambda unit=unit: check_date_trunc_errors(ctx, unit)) for unit in UNITS] +
              [("untaken CASE branch", lambda: check_date_trunc_inside_an_untaken_case_branch(ctx, task_ctx))])


def test_casts(ctx):
    check_casts(ctx)


def test_operators_equal_the_int64_column(ctx, task_ctx):
    cases = []
    for what, units in ((check_compare_in_list_is_null_case, ("s", "ns")), (check_take_filter_concat_slice_sort, ("ms", "us")), (check_group_by_and_accumulators, ("s", "us")),
                        (check_join_keys_and_partitioning, ("s", "ns"))):
        cases += [(f"{what.__name__}[{unit}]", lambda what=what, unit=unit: what(ctx, unit)) for unit in units]
    cases += [("COUNT(DISTINCT)", lambda: check_count_distinct_through_a_plan(ctx, task_ctx)), ("sort-merge join key", lambda: check_sort_merge_join_key(ctx, task_ctx))]
    run_cases(cases)


def test_clickbench_shaped_plans(ctx, task_ctx):
    run_cases([("Q43", lambda: check_q43_shaped_plan(ctx, task_ctx)), ("Q19", lambda: check_q19_shaped_plan(ctx, task_ctx))])
