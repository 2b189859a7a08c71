"""-m gpu: date_part, character_length, substr, left, right and starts_with on the device -- dfgpu_scalar_function (k_date_part, the lane-per-row and
wave-per-row string kernels, k_str_copy, k_starts_with, the dictionary path) and ScalarFunctionExpr through plans.  Expected answers come from
tests/scalar_fn_reference.py, which tests/test_scalar_fn_reference.py pins to the reference's own vectors; every comparison is bit-exact, values and validity."""
import datetime

import numpy as np
import pyarrow as pa
import pytest

import scalar_fn_reference as ref
from test_gpu_expr import exported, same
from views import CLASS_A, CLASS_C, CLASS_C_EDGE, CLASS_E, SPECIAL, ViewCase, plain

pytestmark = pytest.mark.gpu

N = None
ALPHABET = ["a", "ä", "€", "😀"]           # 1, 2, 3 and 4 bytes


def wave_row_bytes(ctx):
    """option string_wave_row_bytes (STR_WAVE_ROW_BYTES of the library): columns averaging this many bytes a row take the wave-per-row kernels"""
    w = ctx.get_option("string_wave_row_bytes")
    assert 16 <= w <= 300, "the shapes below (rows of 0 .. 12 and of 330 .. 380 characters) no longer lie on either side of the threshold"
    return w


# every string kernel gives a row a lane (256 rows per workgroup, a validity / Boolean word per 64 rows) or a wave (4 rows per workgroup): a result word less a
# bit, exactly, a bit more; a workgroup less a row, exactly, a row more; 1000 = full workgroups and a ragged one.  k_date_part takes four days per lane.
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
RESULT_TYPE = {"date_part": pa.float64(), "character_length": pa.int32(), "substr": pa.utf8(), "left": pa.utf8(), "right": pa.utf8(), "starts_with": pa.bool_()}
ARG_TYPES = {"date_part": [pa.utf8(), pa.date32()], "character_length": [pa.utf8()], "substr": [pa.utf8(), pa.int64(), pa.int64()], "left": [pa.utf8(), pa.int64()],
             "right": [pa.utf8(), pa.int64()], "starts_with": [pa.utf8(), pa.utf8()]}


def utf8(values):
    return pa.array(values, type=pa.utf8())


def i64(values):
    return pa.array(values, type=pa.int64())


def date32(days):
    return pa.array(days, type=pa.int32()).cast(pa.date32())


def typed(fn, k, values):
    t = ARG_TYPES[fn][k]
    return date32(values) if t == pa.date32() else pa.array(values, type=t)


def rand_strings(rng, n, null_frac=0.2, lo=0, hi=12, alphabet=ALPHABET):
    lens = rng.integers(lo, hi + 1, n)
    picks = rng.integers(0, len(alphabet), int(lens.sum()))
    out, at = [], 0
    for l in lens:
        out.append("".join(alphabet[j] for j in picks[at:at + l]))
        at += l
    nulls = rng.random(n) < null_frac
    return [None if m else s for s, m in zip(out, nulls)]


def rand_positions(rng, strings, null_frac=0.2, lo=-3):
    """per row a position around the row's own ends: -3 .. 3, length - 3 .. length + 3, or anywhere in between"""
    out = []
    for s in strings:
        l = len(s or "")
        v = int(rng.choice([rng.integers(lo, 4), rng.integers(max(lo, l - 3), l + 4), rng.integers(lo, l + 4)]))
        out.append(None if rng.random() < null_frac else v)
    return out


def call(ctx, fn, args, scalars=None):
    """args: device arrays -> the result as pyarrow (a Utf8 result over a dictionary argument decoded), checked against its own export"""
    out = ctx.scalar_function(ref.FN[fn], args, scalars)
    a = exported(ctx, out)
    assert out.null_count == a.null_count
    return plain(a)


def check(ctx, fn, columns, scalars=None, dev=None, what=""):
    """columns: one Python list per argument (length 1 for a scalar argument); dev: device arrays to use instead of importing the columns"""
    scalars = [False] * len(columns) if scalars is None else scalars
    n = max([len(c) for c, s in zip(columns, scalars) if not s], default=1)
    want = pa.array(ref.rows(fn, [c * n if s else c for c, s in zip(columns, scalars)]), type=RESULT_TYPE[fn])
    args = [ctx.from_arrow(typed(fn, k, c)) if dev is None or dev[k] is None else dev[k] for k, c in enumerate(columns)]
    got = call(ctx, fn, args, scalars)
    assert len(got) == n and same(got, want), f"{fn} {what} scalars={scalars}: got {got.to_pylist()[:8]} want {want.to_pylist()[:8]}"
    return want


def on_device(ctx, fn, columns, scalars=None):
    """the device call alone, for the cases that raise"""
    return call(ctx, fn, [ctx.from_arrow(typed(fn, k, c)) for k, c in enumerate(columns)], scalars)


# ------------------------------------------------------------------ the reference's known answers
GOLDENS = ref.load_goldens()


@pytest.mark.parametrize("fn", sorted(ref.FN))
def test_goldens(ctx, fn):
    """every vector of the function as one-row columns, with every argument a scalar, with the first argument a column and the others scalars, and (strings)
    over a dictionary; a failure names the vector"""
    mine = [c for c in GOLDENS if c["fn"] == fn]
    assert mine
    for case in mine:
        golden_case(ctx, case)


def golden_case(ctx, case):
    import dfgpu
    fn, args = case["fn"], ref.golden_args(case)
    k = len(args)
    cols = [[a] for a in args]
    forms = [[False] * k, [True] * k, [False] + [True] * (k - 1)]
    if fn == "date_part":
        forms = [[True, False], [True, True]]                 # the part name is a scalar
    if "error" in case:
        for sc in forms:
            with pytest.raises(dfgpu.DfgpuError, match=case["error"]) as e:
                on_device(ctx, fn, cols, sc)
            assert e.value.status == 1, case["name"]
        return
    for sc in forms:
        want = check(ctx, fn, cols, sc, what=case["name"])
        assert want.to_pylist() == [case["expected"]], case["name"]
    if fn != "date_part":
        d = ctx.from_arrow(utf8([args[0], "other", args[0]]).dictionary_encode())
        got = call(ctx, fn, [d] + [ctx.from_arrow(typed(fn, j, [args[j]])) for j in range(1, k)], [False] + [True] * (k - 1))
        other = ref.evaluate(fn, ["other"] + args[1:])
        assert same(got, pa.array([case["expected"], other, case["expected"]], type=RESULT_TYPE[fn])), case["name"]


# ------------------------------------------------------------------ row counts, NULLs, both string kernels
def string_cases(rng, strings, null_frac):
    """(fn, columns) for every string function over `strings`, start / count / n as columns around each row's own ends"""
    pos = lambda lo=-3: rand_positions(rng, strings, null_frac, lo)
    prefixes = [None if s is None or rng.random() < null_frac else (s[:int(rng.integers(0, 4))] if rng.random() < 0.7 else "ä" + s[:2]) for s in strings]
    return [("character_length", [strings]), ("substr", [strings, pos()]), ("substr", [strings, pos(), pos(0)]), ("left", [strings, pos()]), ("right", [strings, pos()]),
            ("starts_with", [strings, prefixes])]


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(ctx, n):
    """short: rows of 0 .. 12 characters, the lane-per-row kernels; long: rows of 330 .. 380 characters (at least 330 bytes each), the wave-per-row kernels;
    each without and with NULLs"""
    for shape in ("short", "long"):
        for nulls in (0.0, 0.2):
            lengths_case(ctx, n, shape, nulls)


def lengths_case(ctx, n, shape, nulls):
    rng = np.random.default_rng(1000 + n)
    strings = rand_strings(rng, n, nulls, 0, 12) if shape == "short" else rand_strings(rng, n, 0.0, 330, 380)
    if shape == "long" and nulls:
        strings = [None if rng.random() < nulls else s for s in strings]        # NULL rows hold no bytes: 330 characters a row keep the average above the constant
    if n >= 63 and shape == "long":
        assert sum(len(s.encode()) for s in strings if s is not None) // n >= wave_row_bytes(ctx)
    for fn, cols in string_cases(rng, strings, nulls):
        want = check(ctx, fn, cols, what=f"n={n} {shape} nulls={nulls}")
        assert len(want) == n
    if n:                                                       # scalar start / count / n against the column, and a scalar string against position columns
        check(ctx, "substr", [strings, [2], [3]], [False, True, True])
        check(ctx, "left", [strings, [-2]], [False, True])
        check(ctx, "right", [strings, [3]], [False, True])
        check(ctx, "starts_with", [strings, ["a"]], [False, True])
        check(ctx, "substr", [["aä€😀b"], rand_positions(rng, ["aä€😀b"] * n, nulls), rand_positions(rng, ["aä€😀b"] * n, nulls, 0)], [True, False, False])


def bytes_exactly(rng, nbytes):
    """a string of exactly nbytes bytes over the alphabet"""
    out, left = [], nbytes
    while left:
        c = ALPHABET[int(rng.integers(0, min(left, 4)))]
        out.append(c)
        left -= len(c.encode())
    return "".join(out)


@pytest.mark.parametrize("delta", [-1, 0, 1], ids=["one_below", "at", "one_above"])
def test_rows_around_the_kernel_threshold(ctx, delta):
    """every row has exactly nbytes bytes: one below the threshold the column takes the lane-per-row kernels, at and above it the wave-per-row kernels"""
    nbytes = wave_row_bytes(ctx) + delta
    rng = np.random.default_rng(nbytes)
    strings = [bytes_exactly(rng, nbytes) for _ in range(70)]
    assert all(len(s.encode()) == nbytes for s in strings)
    for fn, cols in string_cases(rng, strings, 0.0):
        check(ctx, fn, cols, what=f"{nbytes} bytes")
    check(ctx, "left", [strings, [3]], [False, True])           # a short row prefix goes to the lane kernel whatever the row length
    check(ctx, "substr", [strings, [1], [2]], [False, True, True])
    check(ctx, "substr", [strings, [-1], [70]], [False, True, True])


@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_each_kernel_on_every_shape(ctx, kernel):
    """the option forces one kernel on short rows, on long rows, on rows of a few KB and on NULLs alike: both kernels see the same data whatever the default is"""
    rng = np.random.default_rng(41)
    saved = ctx.get_option("string_wave_row_bytes")
    ctx.set_option("string_wave_row_bytes", 1 if kernel == "wave" else 1 << 40)
    try:
        for strings in (rand_strings(rng, 300, 0.2, 0, 12), rand_strings(rng, 130, 0.2, 100, 400), ["a" + "€😀ä" * 400 + "b", "", None, "😀" * 17, "x" * 1025]):
            for fn, cols in string_cases(rng, strings, 0.2):
                check(ctx, fn, cols, what=f"forced {kernel}")
            check(ctx, "left", [strings, [3]], [False, True], what=f"forced {kernel}")
            check(ctx, "left", [strings, [40]], [False, True], what=f"forced {kernel}")
            check(ctx, "substr", [strings, [1], [2]], [False, True, True], what=f"forced {kernel}")
            check(ctx, "right", [strings, [5]], [False, True], what=f"forced {kernel}")
    finally:
        ctx.set_option("string_wave_row_bytes", saved)


def test_a_row_of_several_kb(ctx):
    """one row of about 7 KB whose 3- and 4-byte characters lie across the 16-byte chunks of the wave kernel (and the 8-byte words of the lane kernel), in a
    column that is long on average (a wave per row) and in one that is short on average (a lane per row)"""
    big = "a" + ("€😀ä" * 800) + "b"                      # 1 + 9 * 800 + 1 bytes; character k starts at byte 1 + 9 * (k // 3) + (0, 3, 7)[k % 3]: every residue mod 16
    assert len(big.encode()) == 7202 and len(big) == 2402
    rng = np.random.default_rng(7)
    for strings, kind in (([big, "x" * 400, big[5:]], "long"), ([big] + rand_strings(rng, 200, 0.1), "short")):
        nb = sum(len(s.encode()) for s in strings if s) // len(strings)
        assert (nb >= wave_row_bytes(ctx)) == (kind == "long")
        n = len(strings)
        check(ctx, "character_length", [strings])
        for p in (2, 3, 4, 1199, 1200, 1201, 2400, 2401, 2402, 2403):
            check(ctx, "substr", [strings, [p]], [False, True], what=f"{kind} start={p}")
            check(ctx, "substr", [strings, [p], [1000]], [False, True, True], what=f"{kind} start={p}")
            check(ctx, "substr", [strings, [5], [p]], [False, True, True], what=f"{kind} count={p}")
            for q in (p, -p):
                check(ctx, "left", [strings, [q]], [False, True], what=f"{kind} n={q}")
                check(ctx, "right", [strings, [q]], [False, True], what=f"{kind} n={q}")
        check(ctx, "starts_with", [strings, [big[:1500]]], [False, True])
        check(ctx, "starts_with", [strings, [big[:1500] + "a"] * n])


# ------------------------------------------------------------------ every start, count and n over a small set of strings
SMALL = ["", "a", "😀", "aä€😀b", "€€€", "ab😀"]


def test_every_start_count_and_n_as_columns(ctx):
    s2, st2, s3, st3, c3 = [], [], [], [], []
    for s in SMALL:
        r = range(-3, len(s) + 4)
        for a in r:
            s2.append(s); st2.append(a)
            for c in range(0, len(s) + 4):
                s3.append(s); st3.append(a); c3.append(c)
    check(ctx, "substr", [s2, st2])
    check(ctx, "left", [s2, st2])
    check(ctx, "right", [s2, st2])
    want = check(ctx, "substr", [s3, st3, c3])
    assert len(set(want.to_pylist())) > 15


@pytest.mark.parametrize("fn", ["substr2", "substr3", "left", "right"])
def test_every_start_count_and_n_as_scalars(ctx, fn):
    strings = SMALL + [None]
    dev = ctx.from_arrow(utf8(strings))
    top = max(len(s) for s in SMALL) + 3
    for a in range(-3, top + 1):
        if fn == "substr3":
            for c in range(0, top + 1):
                check(ctx, "substr", [strings, [a], [c]], [False, True, True], dev=[dev, None, None], what=f"start={a} count={c}")
        else:
            check(ctx, "substr" if fn == "substr2" else fn, [strings, [a]], [False, True], dev=[dev, None], what=f"{a}")


def test_huge_positions_saturate(ctx):
    strings = SMALL + [None, "x" * 300]
    big = 2**40
    for v in (big, -big):
        check(ctx, "substr", [strings, [v]], [False, True])
        check(ctx, "left", [strings, [v]], [False, True])
        check(ctx, "right", [strings, [v]], [False, True])
        check(ctx, "substr", [strings, [v], [big]], [False, True, True])
        check(ctx, "substr", [strings, [v], [big + 3]], [False, True, True])
        check(ctx, "substr", [strings, [2], [big]], [False, True, True])
    n = len(strings)
    check(ctx, "substr", [strings, [big, -big] * (n // 2), [big + 2] * n])
    check(ctx, "left", [strings, [big, -big] * (n // 2)])
    check(ctx, "right", [strings, [-big, big] * (n // 2)])


# ------------------------------------------------------------------ dates
def day_of(y, m, d):
    return (datetime.date(y, m, d) - datetime.date(1970, 1, 1)).days


_DATES = {}


def date_fixture():
    """the day columns and, per part, their expected values: computed once and shared"""
    if not _DATES:
        rng = np.random.default_rng(2024)
        around = []
        for anchor in (day_of(1, 1, 1), day_of(400, 3, 1), day_of(1600, 3, 1), 0, day_of(9999, 12, 31)):
            around += [d for d in range(anchor - 40, anchor + 41) if ref.MIN_DAY <= d <= ref.MAX_DAY]
        cols = {"span": list(range(day_of(1899, 12, 25), day_of(2101, 1, 5) + 1)), "around": around,
                "random": [int(d) for d in rng.integers(ref.MIN_DAY, ref.MAX_DAY + 1, 20000)]}
        for name, days in cols.items():
            dates = [datetime.date.fromordinal(d + ref.EPOCH_ORDINAL) for d in days]
            iso = [d.isocalendar() for d in dates]
            exp = {"year": [float(d.year) for d in dates], "quarter": [float((d.month - 1) // 3 + 1) for d in dates], "month": [float(d.month) for d in dates],
                   "week": [float(i[1]) for i in iso], "day": [float(d.day) for d in dates], "doy": [float(d.timetuple().tm_yday) for d in dates],
                   "dow": [float((d.weekday() + 1) % 7) for d in dates], "hour": [0.0] * len(days), "epoch": [d * 86400.0 for d in days]}
            _DATES[name] = (days, exp)
        # the table is what scalar_fn_reference.date_part gives: spot-checked here, so that the shortcut above cannot drift from the pinned oracle
        days, exp = _DATES["around"]
        for p in ref.PARTS:
            assert exp[p][::7] == [ref.date_part(p, d) for d in days[::7]]
    return _DATES


@pytest.mark.parametrize("part", ref.PARTS)
def test_date_part(ctx, part):
    """every day from 1899-12-25 to 2101-01-05 (1900 and 2100 are no leap years, 2000 is one; every ISO week 52 / 53 / 1 boundary), 40 days either side of
    0001-01-01, 0400-03-01, 1600-03-01, 1970-01-01 and 9999-12-31, and 20 000 random days of the years 1 to 9999"""
    name = ctx.from_arrow(utf8([part]))
    mixed = ctx.from_arrow(utf8([part[0].upper() + part[1:-1] + part[-1].upper()]))
    for col, (days, exp) in date_fixture().items():
        dev = ctx.from_arrow(date32(days))
        want = pa.array(exp[part], type=pa.float64())
        assert same(call(ctx, "date_part", [name, dev], [True, False]), want), f"{part} over {col}"
        if col == "around":
            assert same(call(ctx, "date_part", [mixed, dev], [True, False]), want)


def test_date_part_lengths_nulls_and_dictionaries(ctx):
    rng = np.random.default_rng(5)
    for n in LENGTHS + [2, 3, 4, 5, 7]:
        days = [int(d) for d in rng.integers(-40000, 60000, n)]
        for nulls in (0.0, 0.3):
            col = [None if rng.random() < nulls else d for d in days]
            for part in ("year", "week", "doy", "epoch"):
                check(ctx, "date_part", [[part], col], [True, False], what=f"n={n}")
    days = [None if rng.random() < 0.2 else int(d) for d in rng.integers(-40000, 60000, 40)]
    codes = pa.array(rng.integers(0, 40, 3000), mask=rng.random(3000) < 0.2).cast(pa.int16())
    arr = pa.DictionaryArray.from_arrays(codes, date32(days))
    for part in ("year", "month", "dow"):
        got = call(ctx, "date_part", [ctx.from_arrow(utf8([part])), ctx.from_arrow(arr)], [True, False])
        want = pa.array([ref.date_part(part, d) for d in plain(arr).cast(pa.int32()).to_pylist()], type=pa.float64())
        assert same(got, want)
    check(ctx, "date_part", [[None], [1, 2, None]], [True, False])             # a NULL part name: every row NULL
    # outside the years 1 .. 9999 nothing is pinned: only that the Int32 extremes run and leave their neighbour alone
    out = ctx.scalar_function(ref.FN["date_part"], [ctx.from_arrow(utf8(["week"])), ctx.from_arrow(date32([2**31 - 1, -2**31, 0]))], [True, False])
    assert out.to_arrow().to_pylist()[2] == 1.0


# ------------------------------------------------------------------ dictionary values
@pytest.mark.parametrize("index_type", [pa.int8(), pa.int32()], ids=["int8", "int32"])
def test_string_functions_over_dictionaries(ctx, index_type):
    """NULL codes and NULL entries; each function runs once per entry; a Utf8 result is a dictionary over the same codes"""
    rng = np.random.default_rng(61)
    n, nd = 3000, 60
    entries = rand_strings(rng, nd, 0.15)
    idx = pa.array(rng.integers(0, nd, n), mask=rng.random(n) < 0.2).cast(index_type)
    arr = pa.DictionaryArray.from_arrays(idx, utf8(entries))
    dev = ctx.from_arrow(arr)
    values = plain(arr).to_pylist()
    check(ctx, "character_length", [values], dev=[dev])
    for v in (-2, 0, 2, 5):
        check(ctx, "substr", [values, [v]], [False, True], dev=[dev, None])
        check(ctx, "substr", [values, [v], [3]], [False, True, True], dev=[dev, None, None])
        check(ctx, "left", [values, [v]], [False, True], dev=[dev, None])
        check(ctx, "right", [values, [v]], [False, True], dev=[dev, None])
    check(ctx, "starts_with", [values, ["aä"]], [False, True], dev=[dev, None])
    check(ctx, "left", [values, [None]], [False, True], dev=[dev, None])
    out = ctx.scalar_function(ref.FN["left"], [dev, ctx.from_arrow(i64([1]))], [False, True])
    assert pa.types.is_dictionary(out.to_arrow().type)


def test_dictionaries_that_are_decoded_first(ctx):
    """a dictionary larger than the column, a dictionary beside another column, a dictionary scalar and a substr whose count can raise are decoded and go row
    by row: the same values, a plain result, and a negative count raises only where the row's code is valid"""
    import dfgpu
    rng = np.random.default_rng(67)
    entries = rand_strings(rng, 100, 0.15)
    n = 70
    idx = pa.array(rng.integers(0, 100, n), mask=rng.random(n) < 0.2).cast(pa.int16())
    arr = pa.DictionaryArray.from_arrays(idx, utf8(entries))
    dev = ctx.from_arrow(arr)
    values = plain(arr).to_pylist()
    check(ctx, "character_length", [values], dev=[dev])
    check(ctx, "left", [values, [2]], [False, True], dev=[dev, None])
    out = ctx.scalar_function(ref.FN["left"], [dev, ctx.from_arrow(i64([2]))], [False, True])
    assert out.to_arrow().type == pa.utf8()                       # decoded: 100 entries for 70 rows
    pos = rand_positions(rng, values, 0.2)
    check(ctx, "substr", [values, pos], dev=[dev, None])
    check(ctx, "substr", [values, pos, rand_positions(rng, values, 0.2, 0)], dev=[dev, None, None])
    check(ctx, "starts_with", [values, ["a"] * n], dev=[dev, None])
    check(ctx, "starts_with", [["aä€"] * n, values], dev=[None, dev])
    one = ctx.from_arrow(utf8(["aä€😀b"]).dictionary_encode())      # a dictionary scalar
    check(ctx, "left", [["aä€😀b"], pos], [True, False], dev=[one, None])
    big = ctx.from_arrow(pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 100, 3000), mask=rng.random(3000) < 0.2).cast(pa.int8()), utf8(entries)))
    bvalues = plain(big.to_arrow()).to_pylist()
    counts = [3] * 3000
    check(ctx, "substr", [bvalues, [1], counts], [False, True, False], dev=[big, None, None])
    bad = next(i for i, v in enumerate(bvalues) if v is not None); null_row = next(i for i, v in enumerate(bvalues) if v is None)
    counts[null_row] = -1
    check(ctx, "substr", [bvalues, [1], counts], [False, True, False], dev=[big, None, None])        # beside a NULL string: no error
    counts[bad] = -1
    with pytest.raises(dfgpu.DfgpuError, match="negative substring length not allowed"):
        ctx.scalar_function(ref.FN["substr"], [big, ctx.from_arrow(i64([1])), ctx.from_arrow(i64(counts))], [False, True, False])
    check(ctx, "substr", [bvalues, [2], [None]], [False, True, True], dev=[big, None, None])          # a NULL literal count cannot raise: once per entry


# ------------------------------------------------------------------ views
VIEWS = [CLASS_A[0], CLASS_A[3], CLASS_C[1], CLASS_C[5], CLASS_C_EDGE[0], CLASS_C_EDGE[1], CLASS_E[0], SPECIAL[0], SPECIAL[1], SPECIAL[3], SPECIAL[4]]


@pytest.mark.parametrize("vc", VIEWS, ids=[v.id for v in VIEWS])
def test_functions_on_views(ctx, vc):
    """Date32 windows (date_part_on_view) and Utf8 windows (offsets[0] > 0, values = the parent's base), validity views whose last word continues with the parent's live bits, the copying slice as
    control; the position and prefix columns are views too.  The pad rows are non-empty and valid, so a row, a word or a byte read outside the window shows."""
    rng = np.random.default_rng(211)
    nf = {"none": 0.0, "clean": 0.0, "some": 0.2, "all": 1.0}[vc.nulls]
    strings = rand_strings(rng, vc.n, nf)
    view, _ = vc.make(ctx, None, rng, arr=utf8(strings))
    a = rand_positions(rng, strings, nf)
    c = rand_positions(rng, strings, nf, 0)
    av, _ = vc.make(ctx, None, rng, arr=i64(a))
    cv, _ = vc.make(ctx, None, rng, arr=i64(c))
    pre = [None if s is None else s[:2] for s in strings]
    pv, _ = vc.make(ctx, None, rng, arr=utf8(pre))
    check(ctx, "character_length", [strings], dev=[view], what=vc.id)
    check(ctx, "substr", [strings, a], dev=[view, av], what=vc.id)
    check(ctx, "substr", [strings, a, c], dev=[view, av, cv], what=vc.id)
    check(ctx, "left", [strings, a], dev=[view, av], what=vc.id)
    check(ctx, "right", [strings, a], dev=[view, av], what=vc.id)
    check(ctx, "starts_with", [strings, pre], dev=[view, pv], what=vc.id)
    if vc.n:
        check(ctx, "substr", [strings, [2], [2]], [False, True, True], dev=[view, None, None], what=vc.id)
        check(ctx, "starts_with", [strings, ["P"]], [False, True], dev=[view, None], what=vc.id)          # the pad rows start with P or 0x7f
        check(ctx, "right", [strings, [2]], [False, True], dev=[view, None], what=vc.id)
    long_strings = [None if s is None else s + "€ä" * 150 for s in strings]                             # and through the wave-per-row kernels
    lview, _ = vc.make(ctx, None, rng, arr=utf8(long_strings))
    check(ctx, "character_length", [long_strings], dev=[lview], what=vc.id + " long")
    check(ctx, "substr", [long_strings, a, c], dev=[lview, av, cv], what=vc.id + " long")
    check(ctx, "right", [long_strings, a], dev=[lview, av], what=vc.id + " long")
    date_part_on_view(ctx, vc)


def date_part_on_view(ctx, vc):
    """a Date32 window at row offset 1 or 3 is not 16-byte aligned (one day per lane), at 64 it is (four days per lane); the pads hold Int32 extremes"""
    rng = np.random.default_rng(223)
    view, exp = vc.make(ctx, "date32", rng)
    days = exp.cast(pa.int32()).to_pylist()
    for part in ("year", "week", "day", "epoch"):
        check(ctx, "date_part", [[part], days], [True, False], dev=[None, view], what=vc.id)


@pytest.mark.parametrize("vc", [CLASS_A[0], CLASS_C[1], CLASS_E[0]], ids=lambda v: v.id)
def test_string_functions_on_dictionary_views(ctx, vc):
    rng = np.random.default_rng(227)
    window = utf8(rand_strings(rng, vc.n, 0.2 if vc.nullable else 0.0, 0, 4, ["a", "ä"])).dictionary_encode()
    view, exp = vc.make(ctx, None, rng, arr=window)
    values = plain(exp).to_pylist()
    check(ctx, "character_length", [values], dev=[view], what=vc.id)
    check(ctx, "left", [values, [2]], [False, True], dev=[view, None], what=vc.id)
    check(ctx, "starts_with", [values, ["PAD"]], [False, True], dev=[view, None], what=vc.id)


# ------------------------------------------------------------------ errors
def test_negative_count(ctx):
    import dfgpu
    f = ctx.from_arrow
    n = 130
    strings = ["aä€😀b"] * n
    ok = [2] * n
    neg = list(ok); neg[70] = -1
    # a negative count beside a NULL string or a NULL start is no error
    s_null = list(strings); s_null[70] = None
    st_null = [1] * n; st_null[70] = None
    check(ctx, "substr", [s_null, [1] * n, neg])
    check(ctx, "substr", [strings, st_null, neg])
    check(ctx, "substr", [[None], [1], [-1]], [True, True, True])
    check(ctx, "substr", [s_null[70:71] * n, [1] * n, [-5]], [False, False, True])
    check(ctx, "substr", [strings, [None], [-5]], [False, True, True])
    # on a valid row it is one, as a column and as a scalar
    for cols, sc in (([strings, [1] * n, neg], None), ([strings, [1] * n, [-1]], [False, False, True]), ([strings, [1], [-1]], [False, True, True])):
        with pytest.raises(dfgpu.DfgpuError, match="negative substring length not allowed") as e:
            on_device(ctx, "substr", cols, sc)
        assert e.value.status == 1
    check(ctx, "substr", [strings, [1] * n, ok])              # the flag does not outlive the call that raised
    # the same row outside the context's row selection does not raise; inside it does
    args = [f(utf8(strings)), f(i64([1] * n)), f(i64(neg))]
    keep = np.ones(n, dtype=bool); keep[70] = False
    mask, other = f(pa.array(keep)), f(pa.array(~keep | (np.arange(n) == 3)))
    try:
        ctx.check(ctx.lib.dfgpu_ctx_set_row_selection(ctx.h, mask.h))
        got = ctx.scalar_function(ref.FN["substr"], args).to_arrow().to_pylist()
        assert [g for i, g in enumerate(got) if i != 70] == ["aä"] * (n - 1)
        ctx.check(ctx.lib.dfgpu_ctx_set_row_selection(ctx.h, other.h))
        with pytest.raises(dfgpu.DfgpuError, match="negative substring length not allowed"):
            ctx.scalar_function(ref.FN["substr"], args)
    finally:
        ctx.check(ctx.lib.dfgpu_ctx_set_row_selection(ctx.h, None))


def test_statuses(ctx):
    import dfgpu
    f = ctx.from_arrow
    d = f(date32([0, 1, 2]))
    s = f(utf8(["a", "b", "c"]))
    one = f(i64([1]))

    def status(fn, args, scalars=None, match=None):
        with pytest.raises(dfgpu.DfgpuError, match=match) as e:
            ctx.scalar_function(fn, args, scalars)
        return e.value.status
    assert status(1, [f(utf8(["fortnight"])), d], [True, False], "Date part 'fortnight' not supported") == 1
    assert status(1, [f(utf8([""])), d], [True, False], "Date part '' not supported") == 1
    for part in ref.UNSUPPORTED_PARTS + ["MINUTE"]:
        assert status(1, [f(utf8([part])), d], [True, False]) == 4
    assert status(1, [f(utf8(["year"] * 3)), d]) == 4                                   # a part name per row
    assert status(1, [f(utf8(["year"])), f(pa.array([0, 1, 2], type=pa.int32()))], [True, False]) == 4      # Int32 is no Date32
    assert status(1, [f(utf8(["year"])), d, d], [True, False, False]) == 4
    assert status(2, [d]) == 4 and status(2, [s, s]) == 4
    assert status(3, [s]) == 4 and status(3, [s, f(pa.array([1], type=pa.int32()))], [False, True]) == 4 and status(3, [s, one, one, one], [False, True, True, True]) == 4
    assert status(4, [s, one, one], [False, True, True]) == 4 and status(5, [s, s]) == 4 and status(6, [s, one], [False, True]) == 4
    assert status(0, [s]) == 4 and status(7, [s]) == 4 and status(99, [s, one], [False, True]) == 4
    assert status(4, [s, f(i64([1, 2]))]) == 5                                          # lengths differ
    from dfgpu import physical_plan as ops
    for fn, k in ((0, 1), (7, 1), (2, 2), (3, 1), (3, 4), (1, 1), (6, 3)):              # refused when the expression is built
        with pytest.raises(dfgpu.DfgpuError) as e:
            ops.ScalarFunctionExpr(fn, [ops.Column("s", 0)] * k).handle(ctx)
        assert e.value.status == 4
    assert status(4, [s, f(i64([1, 2]))], [False, True]) == 5                           # a scalar of length 2


# ------------------------------------------------------------------ ScalarFunctionExpr through plans
def collect_table(plan, task_ctx):
    from dfgpu import physical_plan as ops
    return pa.concat_tables([b.to_arrow() for b in ops.collect(plan, task_ctx)])


def test_q7_shape_year_of_a_date_as_group_key(ctx, task_ctx):
    """TPC-H Q7 / Q8 / Q9: extract(year from l_shipdate) computed by a projection and grouped on"""
    from dfgpu import capi, physical_plan as ops
    rng = np.random.default_rng(307)
    n = 6000
    days = rng.integers(day_of(1992, 1, 1), day_of(1998, 12, 31) + 1, n)
    vol = rng.integers(1, 1000, n).astype(np.float64)
    batch = ops.batch_from_arrow(ctx, pa.table({"l_shipdate": date32(days), "volume": pa.array(vol)}))
    proj = ops.ProjectionExec([(ops.date_part(ops.Literal("year", pa.utf8()), ops.Column("l_shipdate", 0)), "l_year"), (ops.Column("volume", 1), "volume")],
                              ops.MemoryExec([[batch]], batch.schema))
    agg = ops.AggregateExec("Single", [(ops.Column("l_year", 0), "l_year")],
                            [ops.AggregateFunctionExpr("SUM", ops.Column("volume", 1), "revenue", input_field=ops.Field("volume", capi.FLOAT64))], proj)
    out = collect_table(agg, task_ctx)
    years = (days.astype("datetime64[D]").astype("datetime64[Y]").astype(np.int64) + 1970).astype(np.float64)
    assert out.column(0).type == pa.float64()
    assert dict(zip(out.column(0).to_pylist(), out.column(1).to_pylist())) == {float(y): float(vol[years == y].sum()) for y in np.unique(years)}


def test_q22_shape_substring_of_a_phone_number(ctx, task_ctx):
    """TPC-H Q22: substring(c_phone from 1 for 2) in a filter and as a Utf8 group key"""
    from dfgpu import capi, physical_plan as ops
    rng = np.random.default_rng(311)
    n = 5000
    phones = [None if rng.random() < 0.05 else f"{rng.integers(10, 35)}-{rng.integers(100, 999)}-{rng.integers(100, 999)}-{rng.integers(1000, 9999)}" for _ in range(n)]
    bal = rng.integers(-999, 9999, n).astype(np.float64)
    batch = ops.batch_from_arrow(ctx, pa.table({"c_phone": utf8(phones), "c_acctbal": pa.array(bal)}))
    src = lambda: ops.MemoryExec([[batch]], batch.schema)
    L = lambda v: ops.Literal(v, pa.int64())
    code = lambda: ops.substr(ops.Column("c_phone", 0), L(1), L(2))
    f = ops.FilterExec(ops.BinaryExpr(code(), "=", ops.Literal("13", pa.utf8())), src())
    kept = collect_table(f, task_ctx).column(0).to_pylist()
    assert kept == [p for p in phones if p is not None and p[:2] == "13"] and kept
    proj = ops.ProjectionExec([(code(), "cntrycode"), (ops.Column("c_acctbal", 1), "c_acctbal")], src())
    agg = ops.AggregateExec("Single", [(ops.Column("cntrycode", 0), "cntrycode")],
                            [ops.AggregateFunctionExpr("COUNT", ops.Column("c_acctbal", 1), "numcust", input_field=ops.Field("c_acctbal", capi.FLOAT64)),
                             ops.AggregateFunctionExpr("SUM", ops.Column("c_acctbal", 1), "totacctbal", input_field=ops.Field("c_acctbal", capi.FLOAT64))], proj)
    out = collect_table(agg, task_ctx)
    want = {}
    for p, b in zip(phones, bal):
        k = None if p is None else p[:2]
        c, s = want.get(k, (0, 0.0))
        want[k] = (c + 1, s + float(b))
    got = {k: (c, s) for k, c, s in zip(plain(out.column(0).combine_chunks()).to_pylist(), out.column(1).to_pylist(), out.column(2).to_pylist())}
    assert got == want


@pytest.mark.parametrize("encoding", ["plain", "dictionary"])
def test_clickbench_q28_shape_avg_length_of_a_url(ctx, task_ctx, encoding):
    """ClickBench Q28 / Q29: AVG(length("URL")) per key, over a plain and over a dictionary-encoded column"""
    from dfgpu import capi, physical_plan as ops
    rng = np.random.default_rng(313)
    n = 5000
    pool = [None] + ["http://" + "".join(rng.choice(["a", "ä", "/", "€"], int(rng.integers(0, 60)))) for _ in range(80)]
    urls = [pool[j] for j in rng.integers(0, len(pool), n)]
    key = rng.integers(0, 7, n).astype(np.int32)
    col = utf8(urls).dictionary_encode() if encoding == "dictionary" else utf8(urls)
    batch = ops.batch_from_arrow(ctx, pa.table({"k": pa.array(key), "URL": col}))
    arg = ops.character_length(ops.Column("URL", 1))
    as_double = ops.CastExpr(arg, capi.FLOAT64)                    # the planner coerces AVG's argument to Float64
    agg = ops.AggregateExec("Single", [(ops.Column("k", 0), "k")],
                            [ops.AggregateFunctionExpr("AVG", as_double, "l", input_field=ops.Field("l", capi.FLOAT64)),
                             ops.AggregateFunctionExpr("COUNT", arg, "c", input_field=ops.Field("l", capi.INT32))], ops.MemoryExec([[batch]], batch.schema))
    out = collect_table(agg, task_ctx)
    lens = np.array([np.nan if u is None else len(u) for u in urls])
    got = {k: (a, c) for k, a, c in zip(out.column(0).to_pylist(), out.column(1).to_pylist(), out.column(2).to_pylist())}
    want = {}
    for k in np.unique(key):
        v = lens[(key == k) & ~np.isnan(lens)]
        want[int(k)] = (float(v.sum()) / len(v), len(v))              # integer sums below 2^53 divided once, as AVG does
    assert got == want


def test_case_guards_a_substr_that_would_raise(ctx, task_ctx):
    """CASE WHEN n >= 0 THEN substr(s, 1, n) END: the rows with a negative n never reach substr and come out NULL; without the CASE the plan raises"""
    import dfgpu
    from dfgpu import physical_plan as ops
    rng = np.random.default_rng(317)
    n = 3000
    strings = rand_strings(rng, n, 0.1)
    counts = [None if rng.random() < 0.1 else int(v) for v in rng.integers(-3, 8, n)]
    batch = ops.batch_from_arrow(ctx, pa.table({"s": utf8(strings), "n": i64(counts)}))
    src = lambda: ops.MemoryExec([[batch]], batch.schema)
    sub = lambda: ops.substr(ops.Column("s", 0), ops.Literal(1, pa.int64()), ops.Column("n", 1))
    case = ops.CaseExpr(None, [(ops.BinaryExpr(ops.Column("n", 1), ">=", ops.Literal(0, pa.int64())), sub())], None)
    got = collect_table(ops.ProjectionExec([(case, "r")], src()), task_ctx).column(0).combine_chunks()
    want = [None if c is None or c < 0 else ref.substr(s, 1, c, True) for s, c in zip(strings, counts)]
    assert same(got, utf8(want)) and any(c is not None and c < 0 and s is not None for s, c in zip(strings, counts))
    with pytest.raises(dfgpu.DfgpuError, match="negative substring length not allowed"):
        collect_table(ops.ProjectionExec([(sub(), "r")], src()), task_ctx)
    # a filter in front: the rows it dropped do not raise either
    f = ops.FilterExec(ops.BinaryExpr(ops.Column("n", 1), ">=", ops.Literal(0, pa.int64())), src())
    got = collect_table(ops.ProjectionExec([(sub(), "r")], f), task_ctx).column(0).combine_chunks()
    assert same(got, utf8([ref.substr(s, 1, c, True) for s, c in zip(strings, counts) if c is not None and c >= 0]))
