"""CPU: pins the oracle the device tests of CASE use (tests/case_reference.py).  case_rows reproduces every unit-test vector of the reference's
case.rs (tests/golden/case_expr.json), and agrees with pyarrow.compute.case_when -- whose NULL-condition and no-match behaviour is the reference's --
on random cases."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from case_reference import batch_column, case_rows, load_vectors, vector_case_rows

VECTORS = load_vectors()
NAMES = ["case_with_expr", "case_with_expr_else", "case_with_expr_divide_by_zero", "case_without_expr", "case_with_expr_when_null", "case_without_expr_divide_by_zero",
         "case_without_expr_else", "case_with_type_cast", "case_with_matches_and_nulls", "case_expr_matches_and_nulls"]


def test_fixture_holds_the_reference_vectors():
    assert [v["name"] for v in VECTORS] == NAMES
    load4 = batch_column(VECTORS[8])
    assert load4.to_pylist() == [1.77, None, None, 1.78, None, 1.77]
    assert np.frombuffer(load4.buffers()[1], dtype=np.float64)[:3].tolist() == [1.77, 1.77, 1.77]      # the NULL rows keep bytes that match the predicate


@pytest.mark.parametrize("vec", VECTORS, ids=NAMES)
def test_case_rows_on_the_reference_vectors(vec):
    rows, typ = vector_case_rows(vec)
    assert rows == vec["expected"]
    assert pa.array(rows, type=typ).to_pylist() == vec["expected"]


def random_values(rng, kind, n):
    nulls = rng.random(n) < 0.25
    if kind == "int64":
        vals = rng.integers(-2**40, 2**40, n).tolist()
    elif kind == "float64":
        vals = (rng.normal(size=n) * 1e3).tolist()
    elif kind == "bool":
        vals = (rng.random(n) < 0.5).tolist()
    else:
        vals = [["", "a", "BUILDING", "日本語", "x" * 20][j] + str(j) for j in rng.integers(0, 5, n)]
    return [None if m else v for v, m in zip(vals, nulls)]


def test_case_rows_agrees_with_pyarrow_case_when():
    rng = np.random.default_rng(11)
    types = {"int64": pa.int64(), "float64": pa.float64(), "bool": pa.bool_(), "utf8": pa.utf8()}
    for case in range(200):
        kind = ["int64", "float64", "bool", "utf8"][case % 4]
        nb, n, with_else = int(rng.integers(1, 5)), int(rng.integers(1, 40)), bool(rng.integers(0, 2))
        conds = [[None if u < 0.2 else bool(u < 0.5) for u in rng.random(n)] for _ in range(nb)]
        values = [random_values(rng, kind, n) for _ in range(nb)]
        else_ = random_values(rng, kind, n) if with_else else None
        args = [pa.array(v, type=types[kind]) for v in values] + ([pa.array(else_, type=types[kind])] if with_else else [])
        want = pc.case_when(pc.make_struct(*[pa.array(c, type=pa.bool_()) for c in conds]), *args)
        assert case_rows(conds, values, else_) == want.to_pylist(), f"case {case}: {kind}, {nb} branches, else={with_else}"
