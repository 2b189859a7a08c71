"""The oracle of the CASE tests: a first-match loop over Python lists (`to_pylist()` columns), and a reader for the expression
descriptions of tests/golden/case_expr.json (the inputs and expected outputs of the unit tests in the reference's
physical-expr/src/expressions/case.rs).  tests/test_case_reference.py pins both; tests/test_gpu_case.py compares the device with them."""
import json
import math
import os

import pyarrow as pa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "case_expr.json")
PA_TYPES = {"int32": pa.int32(), "int64": pa.int64(), "float64": pa.float64(), "utf8": pa.utf8(), "bool": pa.bool_(), "null": pa.null()}


def case_rows(whens, thens, else_=None):
    """whens[k]: True / False / None per row; thens[k]: values per row, or None for the untyped NULL literal; else_: values per row or None (no ELSE).
    Row i takes thens[k][i] of the first k whose whens[k][i] is True (None counts as False), else else_[i], else None."""
    out = []
    for i in range(len(whens[0])):
        k = next((k for k, w in enumerate(whens) if w[i] is True), None)
        if k is None:
            out.append(else_[i] if else_ is not None else None)
        else:
            out.append(thens[k][i] if thens[k] is not None else None)
    return out


def load_vectors():
    with open(GOLDEN) as f:
        return json.load(f)["vectors"]


def batch_column(vec):
    """the one input column of a vector as a pyarrow array; "validity_bits" puts a validity bitmap over values that stay in the buffer (case_test_batch_nulls)"""
    b = vec["batch"]
    t = PA_TYPES[b["type"]]
    if "validity_bits" not in b:
        return pa.array(b["values"], type=t)
    data = pa.array(b["values"], type=t)
    return pa.Array.from_buffers(t, len(data), [pa.py_buffer(bytes([b["validity_bits"]])), data.buffers()[1]])


def _binary(op, x, y):
    if x is None or y is None:
        return None
    if op == "=":
        return x == y
    if op == ">":
        return x > y
    if op == "/":
        return x / y if y != 0 else math.copysign(math.inf, x)           # Float64 division; the vectors divide positive numbers only
    raise ValueError(op)


def eval_rows(e, column, n):
    """one expression description -> n Python values.  Forms: ["col", name], ["lit", type, value], ["cast", e, type], [op, l, r] with op in = > /"""
    if e[0] == "col":
        return list(column)
    if e[0] == "lit":
        return [e[2]] * n
    if e[0] == "cast":
        conv = {"float64": float, "int32": int}[e[2]]
        return [None if v is None else conv(v) for v in eval_rows(e[1], column, n)]
    return [_binary(e[0], x, y) for x, y in zip(eval_rows(e[1], column, n), eval_rows(e[2], column, n))]


def vector_case_rows(vec):
    """the vector's CASE through case_rows: -> (result rows, result type).  With a base expression WHEN k is `base = when_k`; the ELSE is cast to the type of the THENs."""
    column = batch_column(vec).to_pylist()
    n = len(column)
    base = eval_rows(vec["base"], column, n) if vec.get("base") else None
    whens = []
    for w, _ in vec["when_then"]:
        rows = eval_rows(w, column, n)
        whens.append([_binary("=", b, x) for b, x in zip(base, rows)] if base is not None else rows)
    thens = [eval_rows(t, column, n) for _, t in vec["when_then"]]
    else_ = eval_rows(vec["else"], column, n) if vec.get("else") else None
    if else_ is not None and vec["type"] == "float64":
        else_ = [None if v is None else float(v) for v in else_]
    return case_rows(whens, thens, else_), PA_TYPES[vec["type"]]
