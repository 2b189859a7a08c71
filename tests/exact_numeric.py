"""Exact reference for Decimal128 arithmetic, numeric casts and Decimal128 aggregates, in plain Python integers.

Written from the arrow-arith / arrow-cast 50 and DataFusion rules, not from this project's kernels or its C oracle, so that a mistake
shared by those two does not pass unnoticed.  Semantics restated here:
  - i128 arithmetic is checked on the 128-bit payload (`*_checked`): the declared precision is not enforced by + - * / %.
  - Division truncates toward zero and the remainder takes the dividend's sign (Rust `/` and `%`); i128::MIN / -1 and
    i128::MIN % -1 overflow (`checked_div` / `checked_rem` return None).
  - Decimal result types: add/sub (min(38, max(p1-s1, p2-s2) + max(s1, s2) + 1), max(s1, s2)); mul (min(38, p1+p2+1), s1+s2), an
    error when s1+s2 > 38; div scale min(38, s1+4), the dividend scaled by 10^(scale - s1 + s2) (the divisor by the inverse when that is
    negative), precision min(38, p1 + scale - s1 + s2); rem (min(38, min(p1-s1, p2-s2) + max(s1, s2)), max(s1, s2)).
  - Casts with CastOptions{safe: false}: an unrepresentable value is an error for the whole array.
  - SUM of Decimal128 is add_wrapping (mod 2^128, never an error); AVG is DecimalAverager::avg; MIN / MAX compare as signed i128.

Scales are kept at 22 or below wherever a float is involved: 10^s is exact in an f64 only up to 10^22, and beyond that `powi` and a
multiplication loop may round differently."""
import math
import random

import numpy as np
import pyarrow as pa

I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
U64 = (1 << 64) - 1
MAX_FLOAT_SCALE = 22

INT_RANGES = {pa.int8(): (-(1 << 7), (1 << 7) - 1), pa.int16(): (-(1 << 15), (1 << 15) - 1), pa.int32(): (-(1 << 31), (1 << 31) - 1),
              pa.int64(): (-(1 << 63), (1 << 63) - 1), pa.uint8(): (0, (1 << 8) - 1), pa.uint16(): (0, (1 << 16) - 1),
              pa.uint32(): (0, (1 << 32) - 1), pa.uint64(): (0, (1 << 64) - 1)}


class ArithmeticOverflow(Exception):
    pass


class DivideByZero(Exception):
    pass


class CastError(Exception):
    pass


# ------------------------------------------------------------------------------------------------------------------- i128 helpers
def pow10(k: int) -> int:
    return 10 ** k


def fits128(v: int) -> bool:
    return I128_MIN <= v <= I128_MAX


def wrap128(v: int) -> int:
    v &= (1 << 128) - 1
    return v - (1 << 128) if v >> 127 else v


def _checked(v):
    return v if fits128(v) else None


def add_checked(a: int, b: int):
    return _checked(a + b)


def sub_checked(a: int, b: int):
    return _checked(a - b)


def mul_checked(a: int, b: int):
    return _checked(a * b)


def div_trunc(a: int, b: int) -> int:
    """Rust `a / b`: the quotient truncates toward zero (Python's // floors)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def rem_trunc(a: int, b: int) -> int:
    """Rust `a % b`: the remainder takes the dividend's sign (Python's % takes the divisor's)"""
    return a - b * div_trunc(a, b)


def div_checked(a: int, b: int):
    """i128::checked_div; raises DivideByZero for b == 0, None on overflow (i128::MIN / -1)"""
    if b == 0:
        raise DivideByZero()
    return _checked(div_trunc(a, b))


def rem_checked(a: int, b: int):
    """i128::checked_rem: None for i128::MIN % -1, although the remainder (0) would fit"""
    if b == 0:
        raise DivideByZero()
    if a == I128_MIN and b == -1:
        return None
    return rem_trunc(a, b)


def decimal_fits(v: int, p: int) -> bool:
    return -pow10(p) < v < pow10(p)


def round_half_away(num: int, den: int) -> int:
    """num / den rounded to the nearest integer, ties away from zero (den > 0)"""
    q, r = divmod(abs(num), den)
    if 2 * r >= den:
        q += 1
    return q if num >= 0 else -q


# ------------------------------------------------------------------------------------------------------- decimal arithmetic rules
def decimal_binary_plan(op: str, p1: int, s1: int, p2: int, s2: int):
    """-> (result precision, result scale, left multiplier, right multiplier); ValueError when the result type does not exist"""
    if op in ("+", "-"):
        s = max(s1, s2)
        return min(38, max(p1 - s1, p2 - s2) + s + 1), s, pow10(s - s1), pow10(s - s2)
    if op == "*":
        if s1 + s2 > 38:
            raise ValueError("Output scale of decimal multiply would exceed max scale of 38")
        return min(38, p1 + p2 + 1), s1 + s2, 1, 1
    if op == "/":
        s = min(38, s1 + 4)
        k = s - s1 + s2
        return min(38, p1 + k), s, pow10(k) if k > 0 else 1, pow10(-k) if k < 0 else 1
    if op == "%":
        s = max(s1, s2)
        return min(38, min(p1 - s1, p2 - s2) + s), s, pow10(s - s1), pow10(s - s2)
    raise ValueError(op)


def decimal_binary_value(op: str, x: int, y: int, lm: int, rm: int) -> int:
    """one row of arrow-arith's checked decimal kernel; raises ArithmeticOverflow / DivideByZero"""
    if op != "*":
        x = mul_checked(x, lm)
        if x is None:
            raise ArithmeticOverflow()
        y = mul_checked(y, rm)
        if y is None:
            raise ArithmeticOverflow()
    if op == "+":
        v = add_checked(x, y)
    elif op == "-":
        v = sub_checked(x, y)
    elif op == "*":
        v = mul_checked(x, y)
    elif op == "/":
        v = div_checked(x, y)
    else:
        v = rem_checked(x, y)
    if v is None:
        raise ArithmeticOverflow()
    return v


def decimal_binary(op: str, xs, ys, t1, t2):
    """column op column over lists of ints / None (a scalar is a list of one, broadcast) -> (pa.decimal128 type, values).  The
    whole array fails when any row does; the first failing row decides the kind, as arrow's try_binary stops there."""
    p, s, lm, rm = decimal_binary_plan(op, t1.precision, t1.scale, t2.precision, t2.scale)
    n = max(len(xs), len(ys))
    out = []
    for i in range(n):
        x, y = xs[i if len(xs) > 1 else 0], ys[i if len(ys) > 1 else 0]
        out.append(None if x is None or y is None else decimal_binary_value(op, x, y, lm, rm))
    return pa.decimal128(p, s), out


# ------------------------------------------------------------------------------------------------------------------------------ casts
def int_to_f32(v: int) -> float:
    """an integer rounded once to the nearest f32 (ties to even); returned as the Python float of the same value"""
    a = abs(v)
    e = a.bit_length()
    if e > 24:
        sh = e - 24
        q, r = a >> sh, a & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if r > half or (r == half and q & 1):
            q += 1
        a = q << sh
    if a > 2 ** 128 - 2 ** 104:                                     # above the largest finite f32 after rounding
        return math.copysign(math.inf, v)
    return float(-a if v < 0 else a)


def f64_to_f32(f: float) -> float:
    with np.errstate(over="ignore"):
        return float(np.float32(f))


def cast_value(v, src: pa.DataType, dst: pa.DataType):
    """one non-NULL value of type src cast to dst; raises CastError.  Ints and decimals are Python ints (unscaled for decimals), floats
    are Python floats (a float32 value as its exact double)."""
    if pa.types.is_integer(src):
        if pa.types.is_integer(dst):
            lo, hi = INT_RANGES[dst]
            if not lo <= v <= hi:
                raise CastError()
            return v
        if dst == pa.float64():
            return float(v)
        if dst == pa.float32():
            return int_to_f32(v)
        if pa.types.is_decimal(dst):
            m = mul_checked(v, pow10(dst.scale))
            if m is None or not decimal_fits(m, dst.precision):
                raise CastError()
            return m
    elif pa.types.is_floating(src):
        if dst == pa.float64():
            return v
        if dst == pa.float32():
            return f64_to_f32(v)
        if pa.types.is_integer(dst):
            if not math.isfinite(v):
                raise CastError()
            t = int(v)                                              # exact, truncates toward zero
            lo, hi = INT_RANGES[dst]
            if not lo <= t <= hi:
                raise CastError()
            return t
        if pa.types.is_decimal(dst):
            assert dst.scale <= MAX_FLOAT_SCALE
            m = v * 10.0 ** dst.scale                                # the f64 product, as arrow computes `v * 10f64.powi(s)`
            if not math.isfinite(m):
                raise CastError()
            num, den = m.as_integer_ratio()
            r = round_half_away(num, den)
            if not fits128(r) or not decimal_fits(r, dst.precision):
                raise CastError()
            return r
    elif pa.types.is_decimal(src):
        fs = src.scale
        if pa.types.is_decimal(dst):
            s = dst.scale
            if s >= fs:
                o = mul_checked(v, pow10(s - fs))
                if o is None:
                    raise CastError()
            else:
                o = round_half_away(v, pow10(fs - s))
            if not decimal_fits(o, dst.precision):
                raise CastError()
            return o
        if dst == pa.float64() or dst == pa.float32():
            assert fs <= MAX_FLOAT_SCALE
            f = float(v) / 10.0 ** fs                                # i128 as f64 rounds once; then one IEEE division
            return f if dst == pa.float64() else f64_to_f32(f)
        if pa.types.is_integer(dst):
            t = div_trunc(v, pow10(fs))
            lo, hi = INT_RANGES[dst]
            if not lo <= t <= hi:
                raise CastError()
            return t
    raise ValueError(f"cast {src} -> {dst} is not modelled")


# ------------------------------------------------------------------------------------------------------------------------- aggregates
def sum_type(t: pa.Decimal128Type) -> pa.DataType:
    return pa.decimal128(min(38, t.precision + 10), t.scale)


def avg_type(t: pa.Decimal128Type) -> pa.DataType:
    return pa.decimal128(min(38, t.precision + 4), min(38, t.scale + 4))


def group_sums(values, gids, total):
    """SUM per group: add_wrapping on i128, None for a group that saw no value"""
    acc, cnt = [0] * total, [0] * total
    for v, g in zip(values, gids):
        if v is not None:
            acc[g] += v
            cnt[g] += 1
    return [wrap128(a) if c else None for a, c in zip(acc, cnt)], cnt


def decimal_avg(sum_: int, count: int, sum_scale: int, target_precision: int, target_scale: int) -> int:
    """DecimalAverager::avg (physical-expr/src/aggregate/utils.rs:108-123); raises ArithmeticOverflow"""
    v = mul_checked(sum_, pow10(target_scale - sum_scale))
    if v is None:
        raise ArithmeticOverflow("Arithmetic Overflow in AvgAccumulator")
    q = div_trunc(v, count)
    if not decimal_fits(q, target_precision):
        raise ArithmeticOverflow("Arithmetic Overflow in AvgAccumulator")
    return q


def group_avgs(values, gids, total, t: pa.Decimal128Type):
    sums, cnt = group_sums(values, gids, total)
    at = avg_type(t)
    return [None if c == 0 else decimal_avg(s, c, t.scale, at.precision, at.scale) for s, c in zip(sums, cnt)]


def group_minmax(values, gids, total, is_min: bool):
    out = [None] * total
    for v, g in zip(values, gids):
        if v is not None and (out[g] is None or (v < out[g] if is_min else v > out[g])):
            out[g] = v
    return out


# ---------------------------------------------------------------------------------------------------------- Decimal128 columns, fast
def decimal_array(values, precision: int, scale: int) -> pa.Array:
    """list of ints / None -> Decimal128(precision, scale) through one (lo, hi) uint64 buffer; the values are not checked against the
    precision, as arrow does not check them either"""
    n = len(values)
    words = np.zeros(2 * n, dtype=np.uint64)
    valid = np.ones(n, dtype=bool)
    lo = [0] * n
    hi = [0] * n
    for i, v in enumerate(values):
        if v is None:
            valid[i] = False
        else:
            u = v & ((1 << 128) - 1)
            lo[i], hi[i] = u & U64, u >> 64
    words[0::2] = np.array(lo, dtype=np.uint64)
    words[1::2] = np.array(hi, dtype=np.uint64)
    bitmap = None
    if not valid.all():
        bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.decimal128(precision, scale), n, [bitmap, pa.py_buffer(words.tobytes())], null_count=int((~valid).sum()))


def decimal_values(arr: pa.Array):
    """Decimal128 array -> list of unscaled ints / None, without going through decimal.Decimal"""
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    n = len(arr)
    words = np.frombuffer(arr.buffers()[1], dtype=np.uint64)[2 * arr.offset: 2 * (arr.offset + n)]
    lo, hi = words[0::2].tolist(), words[1::2].tolist()
    valid = np.asarray(arr.is_valid()) if arr.null_count else None
    out = []
    for i in range(n):
        if valid is not None and not valid[i]:
            out.append(None)
        else:
            u = (hi[i] << 64) | lo[i]
            out.append(u - (1 << 128) if u >> 127 else u)
    return out


# ---------------------------------------------------------------------------------------------------------------------- value tables
def edge_table(p: int):
    """the full-width values of a Decimal128(p, _) column that kernels get wrong: word boundaries, low words of 0 and all ones, pairs
    that differ only in one word, the precision's own limits"""
    top = pow10(p) - 1
    base = [0, 1, -1, (1 << 63) - 1, 1 << 63, U64, 1 << 64, (1 << 64) + 1, (1 << 64) | U64, 5 << 64, (5 << 64) | U64, (5 << 64) | 1,
            (6 << 64) | 1, (7 << 64) | U64, (1 << 100) + 12345, (1 << 120) | (1 << 63), top, top - 1, pow10(p - 1), I128_MAX]
    vals = set()
    for v in base:
        for w in (v, -v):
            if abs(w) <= top:
                vals.add(w)
    return sorted(vals)


def random_values(rng: np.random.Generator, n: int, p: int, edge_frac: float = 0.5):
    """about half with a digit count uniform over 1 .. p (log-uniform magnitude up to 10^p - 1) and a random sign, the rest drawn
    from edge_table(p)"""
    edges = edge_table(p)
    r = random.Random(int(rng.integers(0, 1 << 62)))
    out = []
    for _ in range(n):
        if r.random() < edge_frac:
            out.append(edges[r.randrange(len(edges))])
        else:
            d = r.randint(1, p)
            v = r.randrange(pow10(d - 1), pow10(d))
            out.append(-v if r.random() < 0.5 else v)
    return out


def cast_inputs(src: pa.DataType, rng: np.random.Generator, n_random: int = 200):
    """edge table + random draws for a cast from src: a list of Python values (None for NULL) already representable in src"""
    if pa.types.is_decimal(src):
        p, s = src.precision, src.scale
        vals = edge_table(p) + [v for v in (27670116110564333567, -27670116110564333567, (1 << 64) + (1 << 11) + 1) if decimal_fits(v, p)]
        for k in range(1, min(s, 6) + 1):                                  # exact halves (and their neighbours) of every downscale by k digits
            h = 5 * pow10(k - 1)
            for q in (0, 1, 7, pow10(p - k) - 1):
                for d in (-1, 0, 1):
                    v = q * pow10(k) + h + d
                    if decimal_fits(v, p):
                        vals += [v, -v]
        vals += random_values(rng, n_random, p)
    elif pa.types.is_integer(src):
        lo, hi = INT_RANGES[src]
        base = [0, 1, -1, lo, lo + 1, hi, hi - 1, 127, 128, -128, -129, 255, 256, 32767, 32768, -32769, (1 << 31) - 1, 1 << 31, -(1 << 31) - 1,
                (1 << 32) - 1, 1 << 32, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, -(1 << 53) - 1, (1 << 63) - 1, 1 << 63, -(1 << 63),
                4611686843061108735, -4611686843061108735, 9223372036854778879, 9223373686122217471, 999999999999999999, -999999999999999999,
                10 ** 18, 10 ** 19, U64]
        vals = [v for v in base if lo <= v <= hi]
        r = random.Random(int(rng.integers(0, 1 << 62)))
        bits = hi.bit_length()
        vals += [r.randint(lo, hi) for _ in range(n_random // 2)] + [max(lo, min(hi, (r.getrandbits(r.randint(1, bits)) * r.choice((1, -1))))) for _ in range(n_random // 2)]
    else:
        special = [math.nan, math.inf, -math.inf, 0.0, -0.0, 0.5, -0.5, 1 - 2.0 ** -53, -(1 - 2.0 ** -53), 1.5, -1.5, 2.5, -2.5, 0.125, 0.005, -0.005,
                   99.995, -99.995, 1e-7, 12345.678, 2.0 ** 53 - 1, 2.0 ** 53 + 2, -(2.0 ** 53) - 2, 2.0 ** 63, -(2.0 ** 63), 2.0 ** 64, -(2.0 ** 64),
                   4611686843061108735.0, 9223373686122217471.0, 9223372036854778879.0, 1e18, 1e19, 1e20, 1.7e38, -1.7e38, 1e300, 5e-324]
        for lo, hi in INT_RANGES.values():
            for v in (lo, hi):
                for d in (-1, 0, 1):
                    f = float(v + d)
                    special += [f, math.nextafter(f, math.inf), math.nextafter(f, -math.inf)]
        for k in range(0, 39):                                              # around the precision limits 10^k
            f = 10.0 ** k
            special += [f, -f, math.nextafter(f, 0.0), -math.nextafter(f, 0.0)]
        r = np.random.default_rng(int(rng.integers(0, 1 << 62)))
        rnd = (r.standard_normal(n_random) * 10.0 ** r.integers(-4, 25, n_random)).tolist()
        vals = special + rnd
        if src == pa.float32():
            with np.errstate(over="ignore"):
                vals = [float(np.float32(v)) for v in vals]
    out, seen = [], set()
    for v in vals:
        key = (v, math.copysign(1.0, v)) if isinstance(v, float) and not math.isnan(v) else (repr(v),)
        if key not in seen:
            seen.add(key)
            out.append(v)
    return out


def make_column(typ: pa.DataType, values) -> pa.Array:
    """list of Python values / None (unscaled ints for decimals) -> an array of typ"""
    if pa.types.is_decimal(typ):
        return decimal_array(values, typ.precision, typ.scale)
    mask = np.array([v is None for v in values], dtype=bool)
    if pa.types.is_floating(typ):
        data = np.array([0.0 if v is None else v for v in values], dtype=np.float64 if typ == pa.float64() else np.float32)
    else:
        data = np.array([0 if v is None else v for v in values], dtype=typ.to_pandas_dtype())
    return pa.array(data, type=typ, mask=mask if mask.any() else None)


def column_values(arr: pa.Array):
    if pa.types.is_decimal(arr.type):
        return decimal_values(arr)
    return arr.to_pylist()


# ---------------------------------------------------------------------------------------------------- row-by-row check of a kernel
ERROR_KIND = {DivideByZero: "divide by zero", ArithmeticOverflow: "overflow", CastError: "cast"}


def error_kind(exc: BaseException) -> str:
    msg = str(exc).lower()
    if "divide by zero" in msg:
        return "divide by zero"
    if "cast error" in msg or "too large to store" in msg:          # arrow-cast words a precision failure as an invalid argument
        return "cast"
    if "overflow" in msg:
        return "overflow"
    return msg


def same_value(a, b) -> bool:
    if isinstance(a, float) or isinstance(b, float):
        if not (isinstance(a, float) and isinstance(b, float)):
            return False
        if math.isnan(a) or math.isnan(b):
            return math.isnan(a) and math.isnan(b)
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
    return type(a) is type(b) and a == b if isinstance(a, bool) or isinstance(b, bool) else a == b


def expect_rows(fn, n):
    """fn(i) -> the exact value of row i, or raises one of the reference exceptions -> list of values / exception classes"""
    out = []
    for i in range(n):
        try:
            out.append(fn(i))
        except (ArithmeticOverflow, DivideByZero, CastError) as e:
            out.append(type(e))
    return out


def check_rows(run, expect, out_type, raises, max_error_rows: int = 32, label: str = "", always=()):
    """run(rows) evaluates the kernel on a subset of the input rows (a list of indices) and returns a pyarrow array; expect[i] is the
    exact value of row i (None = NULL) or the reference exception class.  The rows that succeed must give exactly the reference values
    and type in one call; the whole input must fail with one of the expected kinds; each failing row (up to max_error_rows of them,
    evenly spread, plus every failing row listed in `always`) must fail on its own with its own kind."""
    n = len(expect)
    is_err = [isinstance(e, type) and issubclass(e, Exception) for e in expect]
    ok = [i for i in range(n) if not is_err[i]]
    err = [i for i in range(n) if is_err[i]]
    if ok:
        got = run(ok)
        assert got.type == out_type, f"{label}: result type {got.type}, expected {out_type}"
        vals = column_values(got)
        bad = [(i, expect[i], v) for i, v in zip(ok, vals) if not same_value(v, expect[i])]
        assert not bad, f"{label}: {len(bad)} of {len(ok)} rows differ from the exact result, first (row, expected, got): {bad[:4]}"
    if err:
        try:
            run(list(range(n)))
        except raises as e:
            kinds = {ERROR_KIND[expect[i]] for i in err}
            assert error_kind(e) in kinds, f"{label}: error {e!r}, expected one of {kinds}"
        else:
            raise AssertionError(f"{label}: no error, but {len(err)} rows must fail (first {err[:4]})")
        step = max(1, len(err) // max_error_rows)
        for i in sorted(set(err[::step][:max_error_rows]) | (set(always) & set(err))):
            try:
                got = run([i])
            except raises as e:
                assert error_kind(e) == ERROR_KIND[expect[i]], f"{label}: row {i}: error {e!r}, expected {ERROR_KIND[expect[i]]}"
            else:
                raise AssertionError(f"{label}: row {i} must fail ({expect[i].__name__}) but gave {column_values(got)}")
    return len(ok), len(err)
