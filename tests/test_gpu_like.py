"""-m gpu: LIKE / NOT LIKE / ILIKE / NOT ILIKE on the device -- dfgpu_like (k_like_anchor, k_like_scan + k_like_resolve, k_like_row, the dictionary path) and
LikeExpr through plans.  Expected answers come from like_rows (tests/like_reference.py, pinned by tests/test_like_reference.py); every comparison is
bit-exact, values and validity."""
import numpy as np
import pyarrow as pa
import pytest

from like_reference import check_golden, golden_patterns, like_rows, load_goldens
from test_gpu_expr import exported, same
from views import CLASS_A, CLASS_C, CLASS_C_EDGE, CLASS_E, SPECIAL, ViewCase

pytestmark = pytest.mark.gpu

ALPHABET = ["a", "b", "A", "B", "k", "s", "K", "ſ", "ä", "%", "_", "\\", "\n"]
FORMS = [(False, False), (True, False), (False, True), (True, True)]          # (negated, case_insensitive): LIKE, NOT LIKE, ILIKE, NOT ILIKE
FORM_IDS = ["like", "not_like", "ilike", "not_ilike"]
TILE = 4096          # LIKE_TILE of like.hip: value bytes per workgroup of k_like_scan
# k_like_anchor / k_like_resolve / k_like_row give every row a lane, 256 rows per workgroup, one ballot per 64 rows: a result word less a bit, exactly, and a
# bit more; a workgroup less a row, exactly, a row more; 1000 = three full workgroups and a ragged fourth.  k_like_scan cuts the value BYTES into tiles of 4096:
# test_like_lengths also runs rows of exactly 16 bytes, so that 255 / 256 / 257 rows are a tile less a row, exactly a tile and a tile plus a row, and 1000 rows
# three full tiles and a ragged fourth.
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]

# one scalar pattern or more of every compiled shape; the comment names the kernel that serves LIKE (ILIKE sends patterns with k or s to k_like_row)
SCALAR_PATTERNS = [
    "ab", "a", "äb",                                      # lit                 k_like_anchor, exact
    "ab%", "B%",                                               # lit%                k_like_anchor
    "%ba", "%ſ",                                          # %lit                k_like_anchor
    "a%b", "ab%ba",                                            # a%b                 k_like_anchor (no middle segment)
    "", "%", "%%",                                             # empty, any          k_like_anchor
    "%ab%", "%a%", "%ä%", "%\n%", "%AB%",                 # %lit%               k_like_scan + k_like_resolve
    "%a%b%", "%ab%ba%", "%aX%Xa%", "%a%%b%",                   # %a%b%
    "a%b%a", "ab%ba%ab", "%a%b",  "a%b%",                      # a%b%c and mixed anchors
    "%k%", "s%", "%ks%b",                                      # letters that fold beyond ASCII under ILIKE
    "a_%", "%_b", "_", "%a_b%", "__%", "_%_",                  # with `_`            k_like_row
    "%\\%%", "\\_%", "%\\\\%", "a\\", "%\\a%", "\\%\\_",       # escapes and plain backslashes
]


def utf8(values):
    return pa.array(values, type=pa.utf8())


def rand_strings(rng, n, null_frac=0.2, lo=0, hi=40, alphabet=ALPHABET):
    lens = rng.integers(lo, hi + 1, n)
    picks = rng.integers(0, len(alphabet), int(lens.sum()))
    out, at = [], 0
    for k, l in enumerate(lens):
        out.append("".join(alphabet[j] for j in picks[at:at + l]))
        at += l
    nulls = rng.random(n) < null_frac
    return [None if m else s for s, m in zip(out, nulls)]


def rand_pattern(rng, case_insensitive):
    alphabet = [c for c in ALPHABET if not (case_insensitive and ord(c) > 127)] + ["%", "%", "_"]
    return "".join(alphabet[j] for j in rng.integers(0, len(alphabet), int(rng.integers(0, 7))))


def run(ctx, dev_values, patterns, negated, case_insensitive):
    """patterns: str / None (a scalar pattern) or a list (a pattern column) -> the result as pyarrow, checked against its own export"""
    scalar = patterns is None or isinstance(patterns, str)
    pat = ctx.from_arrow(utf8([patterns] if scalar else patterns))
    return exported(ctx, ctx.like(dev_values, pat, scalar, negated, case_insensitive))


def check(ctx, values, patterns, negated, case_insensitive, dev_values=None, what=""):
    want = pa.array(like_rows(values, patterns, negated, case_insensitive), type=pa.bool_())
    got = run(ctx, ctx.from_arrow(utf8(values)) if dev_values is None else dev_values, patterns, negated, case_insensitive)
    assert len(got) == len(values) and same(got, want), f"{what} pattern={patterns!r} negated={negated} ilike={case_insensitive}"
    return want


def ascii_only(p):
    return all(ord(c) < 128 for c in p)


# ------------------------------------------------------------------ the reference's known answers
GOLDENS = load_goldens()


@pytest.mark.parametrize("case", GOLDENS, ids=[c["name"] for c in GOLDENS])
def test_like_goldens(ctx, case):
    """column patterns, as the reference's unit test runs them; where all rows share a pattern, the scalar form too; the dictionary query over a dictionary"""
    patterns, scalar = golden_patterns(case)
    n = len(case["values"])
    values = utf8(case["values"])
    dev = ctx.from_arrow(values.dictionary_encode() if case.get("dictionary") else values)
    forms = []
    if not case.get("dictionary"):
        forms.append([patterns] * n if scalar else patterns)
    shared = patterns if scalar else (patterns[0] if len(set(patterns)) == 1 else False)
    if shared is not False:
        forms.append(shared)
    assert forms
    for p in forms:
        got = run(ctx, dev, p, case["negated"], case["case_insensitive"])
        check_golden(case, got.to_pylist())


# ------------------------------------------------------------------ random strings
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_like_scalar_patterns_on_random_strings(ctx, form):
    negated, ci = form
    rng = np.random.default_rng(101)
    values = rand_strings(rng, 2000)
    dev = ctx.from_arrow(utf8(values))
    hits = 0
    for p in SCALAR_PATTERNS:
        if ci and not ascii_only(p):
            continue
        want = check(ctx, values, p, negated, ci, dev)
        hits += want.true_count not in (0, len(values) - want.null_count)
    assert hits > len(SCALAR_PATTERNS) // 2           # most patterns split the rows: the table is not vacuous


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_like_random_scalar_patterns(ctx, form):
    negated, ci = form
    rng = np.random.default_rng(103)
    values = rand_strings(rng, 1500, hi=12)
    dev = ctx.from_arrow(utf8(values))
    for _ in range(40):
        check(ctx, values, rand_pattern(rng, ci), negated, ci, dev)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_like_random_column_patterns(ctx, form):
    negated, ci = form
    rng = np.random.default_rng(107)
    n = 3000
    values = rand_strings(rng, n, hi=10)
    patterns = [None if rng.random() < 0.2 else rand_pattern(rng, ci) for _ in range(n)]
    want = check(ctx, values, patterns, negated, ci)
    assert 0 < want.true_count < n - want.null_count


@pytest.mark.parametrize("n", LENGTHS)
def test_like_lengths(ctx, n):
    rng = np.random.default_rng(n + 1)
    ragged = rand_strings(rng, n, hi=30)
    fixed = rand_strings(rng, n, null_frac=0.0, lo=16, hi=16, alphabet=["a", "b", "k", "x"])       # 16 bytes a row: 256 rows = one tile of k_like_scan
    for values in (ragged, fixed):
        dev = ctx.from_arrow(utf8(values))
        for p in ("%ab%", "%a%b%", "ab%", "%ba", "a%b%a", "%a_b%", "", "%"):
            for negated, ci in FORMS:
                check(ctx, values, p, negated, ci, dev, f"n={n}")
        patterns = [rand_pattern(rng, False) for _ in range(n)]
        check(ctx, values, patterns, False, False, dev, f"n={n} column")
        check(ctx, values, patterns, True, False, dev, f"n={n} column")


def test_like_on_empty_strings_only(ctx):
    """n > 0 rows and not one value byte: nothing may dereference `values`; '%' and '' are true for every valid row"""
    values = ["", None, ""] * 50
    dev = ctx.from_arrow(utf8(values))
    for p in ("%", "", "%%", "a", "%a%", "_", "%_%", "a%b%c"):
        for negated, ci in FORMS:
            want = check(ctx, values, p, negated, ci, dev)
            if p in ("%", "", "%%"):
                assert want.to_pylist() == [None if v is None else not negated for v in values]
    check(ctx, values, [["%", "", "a", None][k % 4] for k in range(len(values))], False, False, dev)
    none = ["", "", ""]                                       # and without a validity buffer
    assert check(ctx, none, "%", False, False).to_pylist() == [True] * 3
    assert check(ctx, none, "%x%", False, False).to_pylist() == [False] * 3


# ------------------------------------------------------------------ tile and row boundaries of the streaming kernels
def cut_stream(buf, keep, step=53, cuts=()):
    """bytes -> rows: a cut every `step` bytes except strictly inside one of the `keep` spans (start, length), plus the extra `cuts`"""
    at = sorted(set(c for c in list(range(step, len(buf), step)) + list(cuts) if not any(s < c < s + l for s, l in keep)))
    rows, prev = [], 0
    for c in at + [len(buf)]:
        rows.append(buf[prev:c].decode())
        prev = c
    return rows


def row_of(rows, pos):
    at = 0
    for k, r in enumerate(rows):
        if at <= pos < at + len(r.encode()):
            return k
        at += len(r.encode())
    raise AssertionError(pos)


STREAM_PATTERNS = ["%special%", "%spec%ial%", "x%special%x", "%special%x", "special%", "%special", "%cial%spe%", "%SPECIAL%"]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_like_match_straddles_every_tile_boundary(ctx, k):
    """A stream of three tiles and a bit: `special` lies across the boundary between tiles 0 / 1 and 1 / 2 with k of its 7 bytes in the tile in front, inside one
    row each time.  A freshly imported column starts on an aligned allocation with offsets[0] = 0, so stream positions are byte offsets."""
    needle = b"special"
    buf = bytearray(b"x" * (3 * TILE + 37))
    spans = [(TILE - k, 7), (2 * TILE - k, 7)]
    for s, l in spans:
        buf[s:s + l] = needle
    rows = cut_stream(bytes(buf), spans)
    dev = ctx.from_arrow(utf8(rows))
    for p in STREAM_PATTERNS:
        for negated, ci in FORMS:
            want = check(ctx, rows, p, negated, ci, dev, f"k={k}")
            if p == "%special%" and not negated:
                assert [i for i, w in enumerate(want.to_pylist()) if w] == [row_of(rows, TILE - k), row_of(rows, 2 * TILE - k)]


def test_like_matches_at_row_edges_and_across_rows(ctx):
    """the needle ends exactly at a row's last byte, begins at a row's first byte (both count), and lies across two adjacent rows (must NOT count) -- the last also
    exactly on a tile boundary, where neither the halo nor the neighbouring tile may turn it into a match"""
    needle = b"special"
    buf = bytearray(b"x" * (3 * TILE + 37))
    ends_row, begins_row, across, across_tile = 500, 1000, 2000, TILE - 3
    for s in (ends_row, begins_row, across, across_tile, 3 * TILE + 37 - 7):
        buf[s:s + 7] = needle
    keep = [(ends_row, 7), (begins_row, 7), (3 * TILE + 30, 7)]
    rows = cut_stream(bytes(buf), keep, cuts=(ends_row + 7, begins_row, across + 4, TILE))
    assert rows[row_of(rows, ends_row)].endswith("special") and rows[row_of(rows, begins_row)].startswith("special") and rows[-1].endswith("special")
    assert rows[row_of(rows, across)].endswith("spec") and rows[row_of(rows, across + 4)].startswith("ial")
    assert rows[row_of(rows, TILE - 1)].endswith("spe") and rows[row_of(rows, TILE)].startswith("cial")
    dev = ctx.from_arrow(utf8(rows))
    for p in STREAM_PATTERNS + ["%spe%cial%", "%x%special"]:
        for negated, ci in FORMS:
            want = check(ctx, rows, p, negated, ci, dev)
            if p == "%special%" and not negated:
                assert [i for i, w in enumerate(want.to_pylist()) if w] == [row_of(rows, ends_row), row_of(rows, begins_row), len(rows) - 1]


@pytest.mark.parametrize("where", ["before", "across", "after"])
def test_like_row_longer_than_a_tile(ctx, where):
    """one row of a tile plus 300 bytes among short rows; it starts 200 bytes into the stream, so the tile boundary at 4096 lies inside it"""
    long_start, long_len = 200, TILE + 300
    pos = {"before": 1000, "across": TILE - 4, "after": TILE + 150}[where]
    body = bytearray(b"y" * long_len)
    body[pos - long_start:pos - long_start + 8] = b"requests"
    body[300:307] = b"special"
    rows = ["short row %d" % k for k in range(10)]
    rows = rows[:5] + ["z" * (long_start - sum(len(r) for r in rows[:5]))] + [body.decode()] + rows[5:] + ["special requests", "requests special", None]
    assert sum(len(r) for r in rows[:6]) == long_start
    dev = ctx.from_arrow(utf8(rows))
    for p in ("%special%requests%", "%requests%", "%requests%special%", "y%special%requests%y", "%special%y%requests%", "%requests", "%special_requests%"):
        for negated, ci in FORMS:
            want = check(ctx, rows, p, negated, ci, dev, where)
            if p == "%special%requests%" and not negated:
                assert want.to_pylist()[6] is True and want.to_pylist()[-3:] == [True, False, None]


def test_like_length_limits_and_overlapping_segments(ctx):
    values = ["ab", "abb", "aXa", "aXXa", "aba", "abaaba", "a", "aa", "", "aaa", "aaaa", "b", None]
    dev = ctx.from_arrow(utf8(values))
    by_pattern = {"ab%b": ["abb"], "%aX%Xa%": ["aXXa"], "aba%aba": ["abaaba"], "a%a": ["aXa", "aXXa", "aba", "abaaba", "aa", "aaa", "aaaa"], "%aa%aa%": ["aaaa"],
                  "abaabaaba": [], "%abaabaaba%": [], "a%b%a%b%a": ["abaaba"]}
    for p, matching in by_pattern.items():
        want = check(ctx, values, p, False, False, dev)
        assert [v for v, w in zip(values, want.to_pylist()) if w] == matching
        for negated, ci in FORMS[1:]:
            check(ctx, values, p, negated, ci, dev)


def test_like_long_patterns(ctx):
    """segments and patterns beyond what the compiled form holds (256 bytes, 6 parts) take the row kernel and give the same answers"""
    rng = np.random.default_rng(109)
    long_lit = "".join(rng.choice(["a", "b"], 300))
    values = [long_lit, "x" + long_lit + "y", long_lit[:-1], "abababab", "a1b2c3d4e5f6g7h8", None, ""]
    dev = ctx.from_arrow(utf8(values))
    for p in ("%" + long_lit + "%", long_lit, long_lit[:200] + "%", "%a%b%a%b%a%b%a%b%", "%1%2%3%4%5%6%7%8", "%" + long_lit[:255] + "%" + long_lit[290:] + "%"):
        for negated, ci in FORMS:
            want = check(ctx, values, p, negated, ci, dev)
        assert want.true_count + want.null_count < len(values)


# ------------------------------------------------------------------ views
VIEW_CASES = [CLASS_A[0], CLASS_A[1], CLASS_A[3], CLASS_C[1], CLASS_C[5], CLASS_C_EDGE[0], CLASS_C_EDGE[1], CLASS_E[0], CLASS_E[1], SPECIAL[0], SPECIAL[1], SPECIAL[3]]
VIEW_PATTERNS = ["%ab%", "%a%b%", "ab%", "%ab", "a%b%a", "%a_b%", "%PAD%", "PAD", "%\x7f%", "%"]


def view_window(vc, rng):
    """the window's rows; the first ones hold the needles, and views.pad_rows puts the window's first non-empty rows around it as poison"""
    frac = {"none": 0.0, "clean": 0.0, "some": 0.2, "all": 1.0}[vc.nulls]
    rows = rand_strings(rng, vc.n, frac, hi=20, alphabet=["a", "b", "A", "k", "x", "ä"])
    for k, s in enumerate(["xxabxx", "ab", "aab", "abxbxa", "axb", "xab"]):
        if k < len(rows) and rows[k] is not None:
            rows[k] = s
    return utf8(rows)


@pytest.mark.parametrize("vc", VIEW_CASES, ids=[v.id for v in VIEW_CASES])
def test_like_on_views(ctx, vc):
    """Utf8 windows (class B: offsets[0] > 0 and odd, values = the parent's base, values_bytes an upper bound), validity views whose last word continues with the
    parent's live bits (class C), the copying slice as control (class E).  The pad rows around the window are non-empty, hold PAD, 0x7f bytes and the window's own
    needle rows, so a read outside the window -- a row too far, or a match found in the stream before offsets[0] or behind offsets[n] -- changes the answer."""
    rng = np.random.default_rng(113)
    window = view_window(vc, rng)
    view, exp = vc.make(ctx, None, rng, arr=window)
    if vc.id == "A-off1":
        parent, off, _ = vc.host(None, rng, arr=window)
        assert int(np.frombuffer(parent.buffers()[1], dtype=np.int32)[off]) % 2 == 1                  # the window's first byte is at an odd offset of the parent's values
    values = exp.to_pylist()
    for p in VIEW_PATTERNS:
        for negated, ci in FORMS:
            if ci and not ascii_only(p):
                continue
            want = check(ctx, values, p, negated, ci, view, vc.id)
            if p in ("%PAD%", "PAD", "%\x7f%") and not negated:
                assert want.true_count == 0                           # only the pad rows hold these
    pv, pexp = vc.make(ctx, None, rng, arr=utf8([rand_pattern(rng, False) for _ in range(vc.n)]))      # a pattern column that is a view too
    check(ctx, values, pexp.to_pylist(), False, False, view, vc.id + " column")
    got = exported(ctx, ctx.like(view, pv, False, True, False))
    assert same(got, pa.array(like_rows(values, pexp.to_pylist(), True, False), type=pa.bool_()))


DICT_VIEW_CASES = [CLASS_A[0], CLASS_A[3], CLASS_C[1], CLASS_C_EDGE[1], CLASS_E[0]]


@pytest.mark.parametrize("vc", DICT_VIEW_CASES, ids=[v.id for v in DICT_VIEW_CASES])
def test_like_on_dictionary_views(ctx, vc):
    """class D: the codes are a window, the dictionary is the parent's (with two PAD entries that only pad codes point at)"""
    rng = np.random.default_rng(127)
    window = view_window(vc, rng).dictionary_encode()
    view, exp = vc.make(ctx, None, rng, arr=window)
    values = exp.dictionary_decode().to_pylist()
    for p in ("%ab%", "%a%b%", "ab%", "%a_b%", "%PAD%", "%"):
        for negated, ci in FORMS:
            check(ctx, values, p, negated, ci, view, vc.id)


# ------------------------------------------------------------------ dictionary values
@pytest.mark.parametrize("index_type", [pa.int8(), pa.int16(), pa.int32()], ids=["int8", "int16", "int32"])
@pytest.mark.parametrize("shape", [(3000, 60), (70, 100)], ids=["dictionary_smaller", "dictionary_larger"])
def test_like_dictionary_values(ctx, index_type, shape):
    """NULL codes and NULL entries; a dictionary smaller than the column goes once per entry and through the codes, a larger one is decoded per row.
    Both give what the decoded column gives."""
    n, nd = shape
    rng = np.random.default_rng(131 + nd)
    entries = rand_strings(rng, nd, null_frac=0.15, hi=12)
    codes = rng.integers(0, nd, n)
    idx = pa.array(codes, mask=rng.random(n) < 0.2).cast(index_type)
    arr = pa.DictionaryArray.from_arrays(idx, utf8(entries))
    decoded = [None if c is None else entries[c] for c in idx.to_pylist()]
    dev = ctx.from_arrow(arr)
    plain_dev = ctx.from_arrow(utf8(decoded))
    for p in ("%ab%", "%a%b%", "a%", "%b", "a%b%a", "%a_b%", "%k%", "", "%", "%\\%%"):
        for negated, ci in FORMS:
            want = check(ctx, decoded, p, negated, ci, dev, f"dictionary {shape}")
            assert same(run(ctx, plain_dev, p, negated, ci), want)
    nonull = pa.DictionaryArray.from_arrays(pa.array(codes).cast(index_type), utf8([e or "" for e in entries]))      # no validity anywhere
    check(ctx, nonull.dictionary_decode().to_pylist(), "%ab%", False, False, ctx.from_arrow(nonull))


# ------------------------------------------------------------------ errors
def test_like_argument_errors(ctx):
    import dfgpu
    f = ctx.from_arrow
    s3, i3, p1, p2 = f(utf8(["a", "b", "c"])), f(pa.array([1, 2, 3])), f(utf8(["a%"])), f(utf8(["a%", "b%"]))
    d3 = f(utf8(["a", "b", "a"]).dictionary_encode())
    di = f(pa.array([1, 2, 1]).dictionary_encode())
    cases = [(lambda: ctx.like(i3, p1), "the value has type"), (lambda: ctx.like(s3, f(pa.array([1]))), "the pattern has type"),
             (lambda: ctx.like(di, p1), "the value has type"), (lambda: ctx.like(s3, d3, False), "the pattern has type"),
             (lambda: ctx.like(s3, p2, False), "operand lengths differ"), (lambda: ctx.like(s3, p2, True), "a scalar pattern must have length 1"),
             (lambda: ctx.like(d3, s3, False), "a dictionary value needs a scalar pattern")]
    for call, message in cases:
        with pytest.raises(dfgpu.DfgpuError, match=message) as e:
            call()
        assert e.value.status == 5
    for values in (s3, d3):
        for pat, scalar in ((f(utf8(["%ä%"])), True), (f(utf8(["a", "ä%", None])), False)):
            if values is d3 and not scalar:
                continue
            with pytest.raises(dfgpu.DfgpuError, match="non-ASCII") as e:
                ctx.like(values, pat, scalar, False, True)
            assert e.value.status == 4
            assert ctx.like(values, pat, scalar, False, False).to_arrow().null_count == (0 if scalar else 1)      # plain LIKE takes the pattern
    with pytest.raises(dfgpu.DfgpuError, match="non-ASCII") as e:                          # a long pattern is checked on the device
        ctx.like(s3, f(utf8(["a" * 300 + "ä"])), True, False, True)
    assert e.value.status == 4
    for values in (s3, d3, f(utf8(["a", None, "c"]))):                                      # a NULL scalar pattern: all NULL, no error
        for negated, ci in FORMS:
            got = exported(ctx, ctx.like(values, f(utf8([None])), True, negated, ci))
            assert same(got, pa.array([None] * 3, type=pa.bool_()))
    assert len(ctx.like(f(utf8([])), p1).to_arrow()) == 0 and len(ctx.like(f(utf8([])), f(utf8([])), False).to_arrow()) == 0


def test_like_under_a_row_selection(ctx):
    """nothing raises per row, so a pushed selection changes nothing: the selected rows equal the unselected evaluation"""
    rng = np.random.default_rng(137)
    values = rand_strings(rng, 1000)
    dev = ctx.from_arrow(utf8(values))
    sel = rng.random(1000) < 0.5
    for p in ("%ab%", "ab%", "%a_b%"):
        want = run(ctx, dev, p, False, False)
        ctx.push_row_selection(ctx.from_arrow(pa.array(sel)))
        try:
            got = run(ctx, dev, p, False, False)
            col = run(ctx, dev, [p] * 1000, False, False)
        finally:
            ctx.pop_row_selection()
        assert same(got.filter(pa.array(sel)), want.filter(pa.array(sel))) and same(col.filter(pa.array(sel)), want.filter(pa.array(sel)))
        assert same(want, pa.array(like_rows(values, p), type=pa.bool_()))


# ------------------------------------------------------------------ LikeExpr through plans
WORDS = ["special", "requests", "packages", "green", "PROMO", "BRASS", "deposits", "accounts", "express", "final"]


def comments(rng, n, null_frac=0.1):
    out = [" ".join(WORDS[j] for j in rng.integers(0, len(WORDS), int(rng.integers(1, 6)))) for _ in range(n)]
    return [None if rng.random() < null_frac else s for s in out]


def collect_table(plan, task_ctx):
    from dfgpu import physical_plan as ops
    return pa.concat_tables([b.to_arrow() for b in ops.collect(plan, task_ctx)])


def S(v):
    from dfgpu import physical_plan as ops
    return ops.Literal(v, pa.utf8())


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_filter_and_projection_over_like(ctx, task_ctx, form):
    from dfgpu import physical_plan as ops
    negated, ci = form
    rng = np.random.default_rng(139)
    n = 3000
    c = comments(rng, n)
    pats = [["%special%", "PROMO%", "%green", "%s%e%", "_____ %"][j] for j in rng.integers(0, 5, n)]
    t = pa.table({"row": pa.array(np.arange(n)), "c": utf8(c), "p": utf8(pats)})
    batch = ops.batch_from_arrow(ctx, t)
    src = lambda: ops.MemoryExec([[batch]], batch.schema)
    for pattern in ("%special%requests%", "promo%", "%BRASS", "%e_press%"):
        e = ops.LikeExpr(ops.Column("c", 1), S(pattern), negated, ci)
        want = like_rows(c, pattern, negated, ci)
        got = collect_table(ops.ProjectionExec([(e, "m")], src()), task_ctx)
        assert same(got.column(0).combine_chunks(), pa.array(want, type=pa.bool_()))
        kept = [r for b in ops.collect(ops.FilterExec(e, src()), task_ctx) for r in b.to_arrow().column(0).to_pylist()]      # `promo%` keeps no row under LIKE: no batch at all
        assert kept == [i for i, w in enumerate(want) if w is True]
    e = ops.LikeExpr(ops.Column("c", 1), ops.Column("p", 2), negated, ci)                 # a pattern that is no literal: one pattern per row
    got = collect_table(ops.ProjectionExec([(e, "m")], src()), task_ctx)
    assert same(got.column(0).combine_chunks(), pa.array(like_rows(c, pats, negated, ci), type=pa.bool_()))
    e = ops.LikeExpr(S("special requests"), ops.Column("p", 2), negated, ci)              # a literal value against a pattern column
    got = collect_table(ops.ProjectionExec([(e, "m")], src()), task_ctx)
    assert same(got.column(0).combine_chunks(), pa.array(like_rows(["special requests"] * n, pats, negated, ci), type=pa.bool_()))


def test_q13_shape_not_like_feeding_an_aggregate(ctx, task_ctx):
    """TPC-H Q13's inner query: orders whose comment is NOT LIKE '%special%requests%', counted per customer"""
    from dfgpu import capi, physical_plan as ops
    rng = np.random.default_rng(149)
    n = 5000
    cust = rng.integers(0, 40, n).astype(np.int64)
    c = comments(rng, n)
    batch = ops.batch_from_arrow(ctx, pa.table({"o_custkey": pa.array(cust), "o_comment": utf8(c), "o_orderkey": pa.array(np.arange(n, dtype=np.int64))}))
    f = ops.FilterExec(ops.LikeExpr(ops.Column("o_comment", 1), S("%special%requests%"), negated=True), ops.MemoryExec([[batch]], batch.schema))
    agg = ops.AggregateExec("Single", [(ops.Column("o_custkey", 0), "o_custkey")],
                            [ops.AggregateFunctionExpr("COUNT", ops.Column("o_orderkey", 2), "c_count", input_field=ops.Field("o_orderkey", capi.INT64))], f)
    out = collect_table(agg, task_ctx)
    keep = np.array([w is True for w in like_rows(c, "%special%requests%", negated=True)])
    assert 0 < keep.sum() < n
    assert dict(zip(out.column(0).to_pylist(), out.column(1).to_pylist())) == {int(k): int((keep & (cust == k)).sum()) for k in np.unique(cust[keep])}


@pytest.mark.parametrize("through_projection", [False, True], ids=["argument", "projection_below"])
def test_q14_shape_sum_of_case_when_like(ctx, task_ctx, through_projection):
    """TPC-H Q14: SUM(CASE WHEN p_type LIKE 'PROMO%' THEN x ELSE 0 END).  fused_aggregate_min_rows = 0 would send the argument to the run-time compiled
    aggregate if LIKE (or CASE) were admitted to it; neither is, so the argument is evaluated node by node -- also when it is a column of the projection below"""
    from dfgpu import capi, physical_plan as ops
    rng = np.random.default_rng(151)
    n = 6000
    types = np.array(["PROMO BRUSHED BRASS", "STANDARD POLISHED TIN", "promo plated steel", "ECONOMY PROMO", "PROMO", "LARGE ANODIZED NICKEL"])[rng.integers(0, 6, n)]
    types = [None if rng.random() < 0.05 else s for s in types]
    x = rng.integers(1, 1000, n).astype(np.float64)
    g = rng.integers(0, 5, n).astype(np.int32)
    batch = ops.batch_from_arrow(ctx, pa.table({"g": pa.array(g), "p_type": utf8(types), "x": pa.array(x)}))
    src = ops.MemoryExec([[batch]], batch.schema)
    case = ops.CaseExpr(None, [(ops.LikeExpr(ops.Column("p_type", 1), S("PROMO%")), ops.Column("x", 2))], ops.Literal(0.0, pa.float64()))
    total = ops.BinaryExpr(ops.Column("x", 2), "*", ops.Literal(1.0, pa.float64()))
    if through_projection:
        src = ops.ProjectionExec([(ops.Column("g", 0), "g"), (case, "promo"), (total, "total")], src)
        args = [ops.Column("promo", 1), ops.Column("total", 2)]
    else:
        args = [case, total]
    aggs = [ops.AggregateFunctionExpr("SUM", args[0], "promo_revenue", input_field=ops.Field("x", capi.FLOAT64)),
            ops.AggregateFunctionExpr("SUM", args[1], "revenue", input_field=ops.Field("x", capi.FLOAT64))]
    saved = ctx.get_option("fused_aggregate_min_rows")
    ctx.set_option("fused_aggregate_min_rows", 0)
    try:
        out = collect_table(ops.AggregateExec("Single", [(ops.Column("g", 0), "g")], aggs, src), task_ctx)
    finally:
        ctx.set_option("fused_aggregate_min_rows", saved)
    promo = np.array([w is True for w in like_rows(types, "PROMO%")])
    assert 0 < promo.sum() < n
    got = {k: (a, b) for k, a, b in zip(out.column(0).to_pylist(), out.column(1).to_pylist(), out.column(2).to_pylist())}
    assert got == {int(k): (float(x[promo & (g == k)].sum()), float(x[g == k].sum())) for k in np.unique(g)}       # integers below 2^53: the sums are exact


def test_like_filter_under_the_probe_side_of_a_join(ctx, task_ctx):
    """LIKE is no `column <op> literal` comparison: with join_probe_fused_filter = 1 the filter is resolved in front of the probe, and the rows equal the
    option-off run and the rows like_rows keeps.  The probe batch has more rows than the TaskContext's batch_size of 8192, the size from which a FilterExec
    under a probe side hands a deferrable predicate on to the join, so the option decides the path a `column <op> literal` filter would take here."""
    from dfgpu import physical_plan as ops
    rng = np.random.default_rng(157)
    nb, npr = 500, 20000
    assert npr > task_ctx.batch_size
    build = pa.table({"b_key": pa.array(np.arange(nb, dtype=np.int64) * 2), "b_val": pa.array(rng.integers(0, 50, nb).astype(np.int32))})
    c = comments(rng, npr, null_frac=0.0)
    probe = pa.table({"p_key": pa.array(rng.integers(0, 2 * nb, npr).astype(np.int64)), "p_comment": utf8(c), "p_row": pa.array(np.arange(npr))})
    mk = lambda t: (lambda b: ops.MemoryExec([[b]], b.schema))(ops.batch_from_arrow(ctx, t))

    def run_plan():
        f = ops.CoalesceBatchesExec(ops.FilterExec(ops.LikeExpr(ops.Column("p_comment", 1), S("%green%")), mk(probe)), 8192)
        j = ops.HashJoinExec(mk(build), f, [(ops.Column("b_key", 0), ops.Column("p_key", 0))], None, "Inner", "CollectLeft")
        return pa.concat_tables([b.to_arrow() for b in j.execute(0, task_ctx)])
    results = []
    for on in (1, 0):
        ctx.set_option("join_probe_fused_filter", on)
        try:
            results.append(run_plan())
        finally:
            ctx.set_option("join_probe_fused_filter", 1)
    assert results[0].equals(results[1]) and results[0].num_rows > 0
    keep = np.array([w is True for w in like_rows(c, "%green%")])
    keys = probe["p_key"].to_numpy()
    want = sorted(int(r) for r in np.flatnonzero(keep & (keys % 2 == 0)))
    assert sorted(results[0]["p_row"].to_pylist()) == want
