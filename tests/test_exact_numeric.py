"""CPU: the exact numeric reference (tests/exact_numeric.py) on hand-computed cases, and the C oracle pinned to it over full-width
Decimal128 edge tables.  The oracle checks most of the suite, so a mistake it shares with the kernels would otherwise pass everywhere."""
import json
import math
import os
import zlib

import numpy as np
import pyarrow as pa
import pytest

import exact_numeric as E
from oracle import pyoracle as po

RNG = np.random.default_rng(4242)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------ the reference itself
def test_i128_wrap_and_checked_ops():
    assert E.wrap128(E.I128_MAX + 1) == E.I128_MIN and E.wrap128(-E.I128_MIN) == E.I128_MIN and E.wrap128(1 << 128) == 0
    assert E.add_checked(E.I128_MAX, 1) is None and E.add_checked(E.I128_MAX, -1) == E.I128_MAX - 1
    assert E.sub_checked(E.I128_MIN, 1) is None and E.sub_checked(-1, E.I128_MAX) == E.I128_MIN
    assert E.mul_checked(1 << 63, 1 << 63) == 1 << 126 and E.mul_checked(1 << 64, 1 << 63) is None
    assert E.mul_checked(-(1 << 64), 1 << 63) == E.I128_MIN and E.mul_checked(E.I128_MIN, -1) is None


@pytest.mark.parametrize("a,b,q,r", [(7, 2, 3, 1), (-7, 2, -3, -1), (7, -2, -3, 1), (-7, -2, 3, -1), (1, 3, 0, 1), (-1, 3, 0, -1),
                                     (E.I128_MIN, 1, E.I128_MIN, 0), (E.I128_MIN + 1, -1, E.I128_MAX, 0), (E.I128_MIN, 2, -(1 << 126), 0),
                                     (E.I128_MIN, E.I128_MAX, -1, -1), (-(10 ** 38) + 1, 10 ** 19, -(10 ** 19) + 1, -(10 ** 19) + 1)])
def test_truncating_division_follows_rust(a, b, q, r):
    assert E.div_checked(a, b) == q and E.rem_checked(a, b) == r


def test_division_overflow_and_zero():
    assert E.div_checked(E.I128_MIN, -1) is None and E.rem_checked(E.I128_MIN, -1) is None
    with pytest.raises(E.DivideByZero):
        E.div_checked(1, 0)
    with pytest.raises(E.DivideByZero):
        E.rem_checked(0, 0)


def test_decimal_result_types():
    # Q1 / Q3: Decimal128(15,2) * (Decimal128(20,0) - Decimal128(15,2)) -> (23,2) then (38,4) (tpch/q1.slt.part)
    assert E.decimal_binary_plan("-", 20, 0, 15, 2)[:2] == (23, 2)
    assert E.decimal_binary_plan("*", 15, 2, 23, 2)[:2] == (38, 4)
    assert E.decimal_binary_plan("/", 10, 2, 10, 2) == (16, 6, 10 ** 6, 1)
    assert E.decimal_binary_plan("/", 38, 38, 38, 0) == (38, 38, 1, 1)
    assert E.decimal_binary_plan("%", 18, 2, 38, 6) == (22, 6, 10 ** 4, 1)
    with pytest.raises(ValueError):
        E.decimal_binary_plan("*", 38, 20, 38, 19)


def test_defect_1_decimal_to_f64_rounds_once():
    v = 27670116110564333567
    assert E.cast_value(v, pa.decimal128(38, 0), pa.float64()) == 27670116110564331520.0
    two_step = float(v >> 64) * 2.0 ** 64 + float(v & E.U64)               # what rounding the low word first gives
    assert two_step == 27670116110564335616.0
    assert E.cast_value(-v, pa.decimal128(38, 0), pa.float64()) == -27670116110564331520.0


def test_defect_2_uint64_to_f64_rounds_once():
    v = 9223372036854778879
    assert E.cast_value(v, pa.uint64(), pa.float64()) == 9223372036854777856.0
    assert float(v - (1 << 64)) + 2.0 ** 64 == 9223372036854779904.0


def test_defect_3_int64_to_f32_rounds_once():
    assert E.cast_value(4611686843061108735, pa.int64(), pa.float32()) == 4611686568183201792.0
    assert E.cast_value(-4611686843061108735, pa.int64(), pa.float32()) == -4611686568183201792.0
    assert E.cast_value(9223373686122217471, pa.uint64(), pa.float32()) == 9223373136366403584.0
    assert float(np.float32(float(4611686843061108735))) == 4611687117939015680.0        # through f64 first: twice
    assert float(np.float32(float(9223373686122217471))) == 9223374235878031360.0
    # the hand rounding agrees with numpy wherever the f64 step is exact
    for v in RNG.integers(-(1 << 53), 1 << 53, 2000).tolist():
        assert E.int_to_f32(v) == float(np.float32(float(v)))
    assert E.int_to_f32((1 << 24) + 1) == float(1 << 24) and E.int_to_f32((1 << 24) + 3) == float((1 << 24) + 4)      # ties to even


@pytest.mark.parametrize("f,to,ok", [(2.0 ** 63, pa.int64(), False), (-(2.0 ** 63), pa.int64(), True), (math.nextafter(-(2.0 ** 63), -math.inf), pa.int64(), False),
                                     (-9.2e18, pa.int64(), True), (-9.25e18, pa.int64(), False), (2.0 ** 64, pa.uint64(), False),
                                     (math.nextafter(2.0 ** 64, 0), pa.uint64(), True), (1.84e19, pa.uint64(), True), (1.845e19, pa.uint64(), False),
                                     (-0.999, pa.uint64(), True), (-1.0, pa.uint64(), False), (math.nan, pa.int8(), False), (math.inf, pa.uint8(), False),
                                     (127.9, pa.int8(), True), (128.0, pa.int8(), False), (-128.9, pa.int8(), True)])
def test_defect_4_float_to_int_exact_limits(f, to, ok):
    if ok:
        assert E.cast_value(f, pa.float64(), to) == int(f)
    else:
        with pytest.raises(E.CastError):
            E.cast_value(f, pa.float64(), to)


def test_decimal_casts_round_half_away_from_zero():
    d = pa.decimal128
    assert E.cast_value(12345, d(5, 3), d(5, 2)) == 1235 and E.cast_value(-12345, d(5, 3), d(5, 2)) == -1235
    assert E.cast_value(12344, d(5, 3), d(5, 2)) == 1234 and E.cast_value(-12344, d(5, 3), d(5, 2)) == -1234
    with pytest.raises(E.CastError):
        E.cast_value(99995, d(5, 3), d(4, 2))                            # 99.995 -> 100.00 needs 5 digits
    assert E.cast_value(99994, d(5, 3), d(4, 2)) == 9999
    assert E.cast_value(2.5, pa.float64(), d(10, 0)) == 3 and E.cast_value(-2.5, pa.float64(), d(10, 0)) == -3
    assert E.cast_value(0.125, pa.float64(), d(10, 2)) == 13 and E.cast_value(-0.125, pa.float64(), d(10, 2)) == -13
    assert E.cast_value(-1999, d(38, 3), pa.int8()) == -1 and E.cast_value(10 ** 20 - 1, d(38, 0), d(38, 18)) == (10 ** 20 - 1) * 10 ** 18
    with pytest.raises(E.CastError):
        E.cast_value(10 ** 20, d(38, 0), d(38, 18))


def test_decimal_avg_and_sum_rules():
    t = pa.decimal128(38, 2)
    assert E.decimal_avg(-7, 2, 2, 38, 6) == -35000                      # -0.035 exactly
    assert E.decimal_avg(-1, 3, 2, 38, 6) == -3333                       # truncates toward zero
    with pytest.raises(E.ArithmeticOverflow, match="AvgAccumulator"):
        E.decimal_avg(10 ** 35, 1, 2, 38, 6)                             # only the 10^4 rescale overflows
    sums, _ = E.group_sums([E.I128_MAX, 1, None], [0, 0, 1], 2)
    assert sums == [E.I128_MIN, None]
    assert E.group_avgs([1, 2, None], [0, 0, 0], 1, t) == [15000]


def test_reference_agrees_with_the_golden_aggregate_vectors():
    golden = json.load(open(os.path.join(GOLDEN, "aggregates.json")))
    used = 0
    for case in golden["scalar"]:
        if case.get("func") not in ("SUM", "AVG") or not isinstance(case.get("type"), dict):
            continue
        t = pa.decimal128(*case["type"]["decimal128"])
        vals = case["values"]
        exp_t = pa.decimal128(*case["expected_type"]["decimal128"])
        fn = E.sum_type if case["func"] == "SUM" else E.avg_type
        assert fn(t) == exp_t, case["name"]
        got = (E.group_sums(vals, [0] * len(vals), 1)[0] if case["func"] == "SUM" else E.group_avgs(vals, [0] * len(vals), 1, t))[0]
        assert got == case["expected"], case["name"]
        used += 1
    assert used >= 4


def test_decimal_column_builder_round_trips():
    vals = E.random_values(RNG, 5000, 38) + [None, E.I128_MIN, E.I128_MAX]
    a = E.decimal_array(vals, 38, 5)
    assert a.null_count == 1 and E.decimal_values(a) == vals
    assert E.decimal_values(a.slice(7, 100)) == vals[7:107]
    small = [v for v in vals if v is not None and abs(v) < 10 ** 38]
    import decimal
    assert a.to_pylist()[:50] == [None if v is None else decimal.Decimal(v).scaleb(-5, context=decimal.Context(prec=60)) for v in vals[:50]]
    assert any(abs(v) >= 1 << 64 for v in small) and any(0 < abs(v) < 1 << 63 for v in small)


# ----------------------------------------------------------------------------------------------- the oracle, pinned to the reference
DEC_BINARY_TYPES = [((38, 0), (38, 0)), ((38, 10), (38, 10)), ((38, 10), (20, 0)), ((18, 2), (38, 6)), ((38, 0), (38, 10))]


def binary_inputs(t1, t2, n_random=300):
    xs = E.edge_table(t1.precision) + E.random_values(RNG, n_random, t1.precision) + [None]
    ys = E.edge_table(t2.precision) + E.random_values(RNG, n_random, t2.precision) + [None]
    xs2 = [x for x in xs for _ in range(2)]
    ys2 = (ys * (len(xs2) // len(ys) + 1))[:len(xs2)]
    RNG.shuffle(ys2)
    ex, ey = E.edge_table(t1.precision), E.edge_table(t2.precision)
    xs2 += [x for x in ex for _ in ey]                                   # every pair of edges
    ys2 += [y for _ in ex for y in ey]
    return xs2, ys2


def oracle_binary(op, xs, ys, t1, t2, ls=False, rs=False):
    def run(rows):
        l = E.make_column(t1, xs if ls else [xs[i] for i in rows])
        r = E.make_column(t2, ys if rs else [ys[i] for i in rows])
        return po.binary(op, l, r, l_scalar=ls, r_scalar=rs)
    return run


@pytest.mark.parametrize("op", ["+", "-", "*", "/", "%"])
@pytest.mark.parametrize("types", DEC_BINARY_TYPES, ids=[f"{a}x{b}" for a, b in DEC_BINARY_TYPES])
def test_oracle_decimal_binary_equals_exact(op, types):
    t1, t2 = pa.decimal128(*types[0]), pa.decimal128(*types[1])
    xs, ys = binary_inputs(t1, t2)
    p, s, lm, rm = E.decimal_binary_plan(op, t1.precision, t1.scale, t2.precision, t2.scale)
    exp = E.expect_rows(lambda i: None if xs[i] is None or ys[i] is None else E.decimal_binary_value(op, xs[i], ys[i], lm, rm), len(xs))
    E.check_rows(oracle_binary(op, xs, ys, t1, t2), exp, pa.decimal128(p, s), po.OracleError, max_error_rows=200, label="oracle")
    for sc in (E.I128_MIN + 1, -1, 0, (1 << 64) + 1, 10 ** 19):          # a scalar on each side
        exp = E.expect_rows(lambda i: None if ys[i] is None else E.decimal_binary_value(op, sc, ys[i], lm, rm), len(ys))
        E.check_rows(oracle_binary(op, [sc], ys, t1, t2, ls=True), exp, pa.decimal128(p, s), po.OracleError, max_error_rows=50, label=f"oracle {sc} {op} col")
        exp = E.expect_rows(lambda i: None if xs[i] is None else E.decimal_binary_value(op, xs[i], sc, lm, rm), len(xs))
        E.check_rows(oracle_binary(op, xs, [sc], t1, t2, rs=True), exp, pa.decimal128(p, s), po.OracleError, max_error_rows=50, label=f"oracle col {op} {sc}")


def test_oracle_decimal_multiply_scale_39_fails():
    t1, t2 = pa.decimal128(38, 20), pa.decimal128(38, 19)
    with pytest.raises(po.OracleError):
        po.binary("*", E.make_column(t1, [1]), E.make_column(t2, [1]))


@pytest.mark.parametrize("op", ["/", "%"])
def test_oracle_i128_min_by_minus_one_overflows(op):
    t1 = pa.decimal128(38, 38) if op == "/" else pa.decimal128(38, 0)         # the only types whose dividend is not rescaled
    t2 = pa.decimal128(38, 0)
    xs = [E.I128_MIN, E.I128_MIN, E.I128_MIN + 1, E.I128_MIN + 1, E.I128_MAX, E.I128_MIN]
    ys = [-1, 1, -1, 1, -1, 2]
    p, s, lm, rm = E.decimal_binary_plan(op, t1.precision, t1.scale, t2.precision, t2.scale)
    assert lm == rm == 1
    exp = E.expect_rows(lambda i: E.decimal_binary_value(op, xs[i], ys[i], lm, rm), len(xs))
    assert exp[0] is E.ArithmeticOverflow
    E.check_rows(oracle_binary(op, xs, ys, t1, t2), exp, pa.decimal128(p, s), po.OracleError, label="oracle")


CMP_OPS = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


@pytest.mark.parametrize("op", list(CMP_OPS))
def test_oracle_decimal_comparisons_full_width(op):
    t = pa.decimal128(38, 6)
    e = E.edge_table(38)
    xs = [x for x in e for _ in e] + [None, 1]
    ys = [y for _ in e for y in e] + [1, None]
    exp = [None if x is None or y is None else CMP_OPS[op](x, y) for x, y in zip(xs, ys)]
    got = po.binary(op, E.make_column(t, xs), E.make_column(t, ys))
    assert got.to_pylist() == exp


CAST_SOURCES = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(), pa.float32(), pa.float64(),
                pa.decimal128(38, 0), pa.decimal128(38, 10), pa.decimal128(18, 2), pa.decimal128(5, 3)]
CAST_TARGETS = [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(), pa.float32(), pa.float64(),
                pa.decimal128(38, 0), pa.decimal128(38, 10), pa.decimal128(18, 4), pa.decimal128(4, 2), pa.decimal128(38, 22)]


def cast_cases():
    return [(s, t) for s in CAST_SOURCES for t in CAST_TARGETS if s != t or pa.types.is_decimal(s)]


def cast_check(run_cast, src, dst, raises, max_error_rows):
    """every failing edge value is also run on its own; of the random draws, a spread sample"""
    seed = zlib.crc32(f"{src}->{dst}".encode())
    n_edge = len(E.cast_inputs(src, np.random.default_rng(seed), n_random=0))
    vals = E.cast_inputs(src, np.random.default_rng(seed)) + [None]
    exp = E.expect_rows(lambda i: None if vals[i] is None else E.cast_value(vals[i], src, dst), len(vals))
    return E.check_rows(lambda rows: run_cast(E.make_column(src, [vals[i] for i in rows]), dst), exp, dst, raises, max_error_rows=max_error_rows,
                        label=f"cast {src} -> {dst}", always=range(n_edge))


@pytest.mark.parametrize("src,dst", cast_cases(), ids=[f"{s}->{t}" for s, t in cast_cases()])
def test_oracle_cast_equals_exact(src, dst):
    cast_check(po.cast, src, dst, po.OracleError, 1000)


@pytest.mark.parametrize("p,s", [(38, 2), (18, 2)])
def test_oracle_accumulators_equal_exact(p, s):
    t = pa.decimal128(p, s)
    total = 97
    vals = E.random_values(RNG, 20000, p) + [None] * 50
    gids = RNG.integers(0, total, len(vals))
    arr = E.make_column(t, vals)
    for kind in ("SUM", "MIN", "MAX", "AVG"):
        exp_t = E.sum_type(t) if kind == "SUM" else E.avg_type(t) if kind == "AVG" else t
        rows = np.ones(len(vals), dtype=bool)
        if kind == "AVG":
            sums, cnt = E.group_sums(vals, gids.tolist(), total)
            want = E.expect_rows(lambda g: None if cnt[g] == 0 else E.decimal_avg(sums[g], cnt[g], s, exp_t.precision, exp_t.scale), total)
            bad = [g for g in range(total) if isinstance(want[g], type)]
            if bad:                                                       # a full-width group sum overflows the 10^4 rescale: an error
                acc = po.Acc(kind, t)
                acc.update_batch(arr, gids, None, total)
                with pytest.raises(po.OracleError, match="AvgAccumulator"):
                    acc.evaluate()
                rows = ~np.isin(gids, bad)
                want = [None if g in bad else w for g, w in enumerate(want)]
        elif kind == "SUM":
            want = E.group_sums(vals, gids.tolist(), total)[0]
        else:
            want = E.group_minmax(vals, gids.tolist(), total, kind == "MIN")
        acc = po.Acc(kind, t)
        acc.update_batch(arr.filter(pa.array(rows)), gids[rows], None, total)
        got = acc.evaluate()
        assert got.type == exp_t
        assert E.decimal_values(got) == want, kind
