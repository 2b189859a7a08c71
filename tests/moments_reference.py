"""Plain-Python restatement of the reference's VarianceAccumulator / StddevAccumulator (physical-expr/src/aggregate/variance.rs:202-333, stddev.rs:202-241) with Python
floats (IEEE binary64) in the reference's operation order, grouped the way GroupsAccumulatorAdapter feeds them: every group has an accumulator of its own that sees its
rows in input order, batch by batch.  Also: exact rational answers (fractions.Fraction) to measure the model's and the device's error against, and the generators of the
random inputs that tests/test_variance_stddev.py runs on the device and tests/test_moments_reference.py checks the model on."""
import decimal
import math
from fractions import Fraction

import numpy as np

KINDS = ("VAR_SAMP", "VAR_POP", "STDDEV_SAMP", "STDDEV_POP")
GID_NONE = 0xFFFFFFFF
NUMPY_TYPES = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64, "uint8": np.uint8, "uint16": np.uint16, "uint32": np.uint32, "uint64": np.uint64,
               "float32": np.float32, "float64": np.float64}


def as_f64(v, dtype="float64"):
    """arrow-cast's `as f64` of one value of `dtype` (variance.rs:243)"""
    if dtype == "float32":
        return float(np.float32(v))
    if dtype == "float64":
        return float(v)
    return float(int(v))                    # correctly rounded for every 64-bit integer, like `as f64`


class VarianceAccumulator:
    def __init__(self):
        self.count, self.mean, self.m2 = 0, 0.0, 0.0                       # variance.rs:211-218

    def update_batch(self, values, dtype="float64"):                        # :242-259
        for v in values:
            if v is None:
                continue
            value = as_f64(v, dtype)
            new_count = self.count + 1
            delta1 = value - self.mean
            new_mean = delta1 / float(new_count) + self.mean
            delta2 = value - new_mean
            new_m2 = self.m2 + delta1 * delta2
            self.count += 1
            self.mean = new_mean
            self.m2 = new_m2

    def merge_batch(self, counts, means, m2s):                              # :280-303
        for c, mean, m2 in zip(counts, means, m2s):
            if c == 0:
                continue
            new_count = self.count + c
            new_mean = self.mean * float(self.count) / float(new_count) + mean * float(c) / float(new_count)
            delta = self.mean - mean
            new_m2 = self.m2 + m2 + delta * delta * float(self.count) * float(c) / float(new_count)
            self.count = new_count
            self.mean = new_mean
            self.m2 = new_m2

    def state(self):                                                        # :234-240
        return (self.count, self.mean, self.m2)

    def evaluate(self, kind):                                               # :305-328, stddev.rs:223-232
        population = kind in ("VAR_POP", "STDDEV_POP")
        count = self.count if population else (self.count - 1 if self.count > 0 else self.count)
        if self.count == 0:
            v = None
        elif self.count == 1:
            v = 0.0 if population else None
        else:
            v = self.m2 / float(count)
        if v is not None and kind.startswith("STDDEV"):
            v = math.sqrt(v) if v >= 0.0 else (v if v == 0.0 else float("nan"))       # f64::sqrt: NaN for NaN and for negatives
        return v


def passes(gid, i, opt_filter):
    return gid != GID_NONE and (opt_filter is None or opt_filter[i] is True)


class GroupedMoments:
    """GroupsAccumulatorAdapter over VarianceAccumulator: one accumulator per group"""

    def __init__(self, kind="VAR_SAMP", dtype="float64"):
        self.kind, self.dtype, self.accs = kind, dtype, []

    def _grow(self, total):
        while len(self.accs) < total:
            self.accs.append(VarianceAccumulator())

    def update_batch(self, values, gids, opt_filter, total):
        self._grow(total)
        for i, (v, g) in enumerate(zip(values, gids)):
            if passes(g, i, opt_filter):
                self.accs[g].update_batch([v], self.dtype)

    def merge_batch(self, states, gids, opt_filter, total):
        self._grow(total)
        counts, means, m2s = states
        for i, g in enumerate(gids):
            if passes(g, i, opt_filter):
                self.accs[g].merge_batch([counts[i]], [means[i]], [m2s[i]])

    def state(self):
        return [a.count for a in self.accs], [a.mean for a in self.accs], [a.m2 for a in self.accs]

    def evaluate(self, kind=None):
        return [a.evaluate(kind or self.kind) for a in self.accs]


# ------------------------------------------------------------------ exact arithmetic
def group_values(batches, dtype="float64"):
    """the values every group receives from update batches, as exact Fractions of their `as f64` casts"""
    total = max([b["total"] for b in batches] + [0])
    out = [[] for _ in range(total)]
    for b in batches:
        for i, (v, g) in enumerate(zip(b["values"], b["gids"])):
            if v is not None and passes(g, i, b.get("filter")):
                out[g].append(Fraction(as_f64(v, dtype)))
    return out


def exact_state(xs):
    """(count, mean, m2) of exact values, as Fractions"""
    n = len(xs)
    if n == 0:
        return 0, Fraction(0), Fraction(0)
    s = sum(xs, Fraction(0))
    return n, s / n, sum((x * x for x in xs), Fraction(0)) - s * s / n


def exact_evaluate(kind, xs):
    """None, or the exact answer as a decimal.Decimal of 60 digits"""
    n, _, m2 = exact_state(xs)
    population = kind in ("VAR_POP", "STDDEV_POP")
    if n == 0 or (n == 1 and not population):
        return None
    with decimal.localcontext() as c:
        c.prec = 60
        if n == 1:
            return decimal.Decimal(0)
        v = m2 / (n if population else n - 1)
        d = decimal.Decimal(v.numerator) / decimal.Decimal(v.denominator)
        return d.sqrt() if kind.startswith("STDDEV") else d


def rel_err(got, exact):
    """|got - exact| / |exact| of a float against a Decimal (0.0 when both are zero)"""
    with decimal.localcontext() as c:
        c.prec = 60
        e = decimal.Decimal(exact); d = abs(decimal.Decimal(got) - e)
        if d == 0:
            return 0.0
        return float("inf") if e == 0 else float(d / abs(e))


# ------------------------------------------------------------------ the random inputs of the device tests
MOMENTS_LDS_GROUPS = 1024          # T: the largest number of groups the LDS path of csrc/moments.hip takes (MOMENTS_LDS_GROUPS there)
PATH_ROWS = (0, 1, 63, 64, 65, 255, 257, 4097)
PATH_TOTALS = (1, 2, 9, MOMENTS_LDS_GROUPS, MOMENTS_LDS_GROUPS + 1, 5000)


def normal_values(rng, gids, total):
    """|mean| / sd <= 10: group g draws from N(mean_g, 1) with mean_g uniform in [-10, 10]"""
    means = rng.uniform(-10.0, 10.0, max(total, 1))
    g = np.asarray(gids, dtype=np.int64)
    return (means[np.minimum(g, max(total, 1) - 1)] + rng.standard_normal(len(g))).tolist()


def batch(values, gids, total, opt_filter=None):
    return {"values": list(values), "gids": [int(g) for g in gids], "filter": opt_filter, "total": int(total)}


def path_batch(n, total, ids="random"):
    """one update batch of n rows over `total` groups: random ids (some groups get no row), all-equal ids (every wave uniform) or strictly alternating ids (no wave uniform)"""
    rng = np.random.default_rng(1000 * n + total + {"random": 0, "equal": 7, "alternating": 13}[ids])
    if ids == "random":
        gids = rng.integers(0, total, n)
    elif ids == "equal":
        gids = np.full(n, total - 1)
    else:
        gids = np.arange(n) % 2 * (total - 1)
    return batch(normal_values(rng, gids, total), gids, total)


def nulls_filters_batch(n=1500, total=37, seed=21):
    """30 % NULL values, a filter with false and NULL entries, ids of 0xFFFFFFFF"""
    rng = np.random.default_rng(seed)
    gids = rng.integers(0, total, n)
    values = normal_values(rng, gids, total)
    values = [None if r < 0.3 else v for v, r in zip(values, rng.random(n))]
    filt = [[True, True, True, False, None][k] for k in rng.integers(0, 5, n)]
    gids = [GID_NONE if r < 0.1 else int(g) for g, r in zip(gids, rng.random(n))]
    return batch(values, gids, total, filt)


def three_batches(seed=33):
    """new groups appear in batches 2 and 3 and the total grows across MOMENTS_LDS_GROUPS"""
    rng = np.random.default_rng(seed)
    out = []
    for n, total in ((300, 5), (700, 11), (4000, MOMENTS_LDS_GROUPS + 76)):
        gids = rng.integers(0, total, n)
        out.append(batch(normal_values(rng, gids, total), gids, total))
    return out


def merge_inputs(total=300, seed=44):
    """the update batches of two accumulators whose states are merged into a third"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (2500, 1700):
        gids = rng.integers(0, total, n)
        values = normal_values(rng, gids, total)
        out.append(batch([None if r < 0.1 else v for v, r in zip(values, rng.random(n))], gids, total))
    return out


def typed_batch(dtype, n=600, total=13, seed=55):
    """values of `dtype` over its whole range (UInt64: above 2^63 too; floats: normal around a per-group mean)"""
    rng = np.random.default_rng(seed + len(dtype) + ord(dtype[0]) + ord(dtype[-1]))
    gids = rng.integers(0, total, n)
    if dtype.startswith("float"):
        values = [NUMPY_TYPES[dtype](v).item() for v in normal_values(rng, gids, total)]
    else:
        info = np.iinfo(NUMPY_TYPES[dtype])
        values = [int(v) for v in rng.integers(info.min, info.max, n, dtype=NUMPY_TYPES[dtype], endpoint=True)]
    return batch(values, gids, total)


def plan_tables(seed=5, batches=3, rows=4000, groups=40):
    """the plan-level input: per batch the columns k (Int64 key, 5 % NULL), x (Float64 multiples of 1/64, 20 % NULL), f (Boolean FILTER column with false and NULL entries)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batches):
        k = rng.integers(0, groups, rows)
        x = [round(v * 64.0) / 64.0 for v in normal_values(rng, k, groups)]            # multiples of 1/64: their Float64 SUM is exact in any order
        out.append({"k": [None if r < 0.05 else int(v) for v, r in zip(k, rng.random(rows))],
                    "x": [None if r < 0.2 else v for v, r in zip(x, rng.random(rows))],
                    "f": [[True, True, False, None][j] for j in rng.integers(0, 4, rows)]})
    return out


def first_seen_ids(keys, table=None):
    """group ids in first-seen order of the keys (None is a key of its own) -> (ids, table)"""
    table = {} if table is None else table
    ids = []
    for key in keys:
        if key not in table:
            table[key] = len(table)
        ids.append(table[key])
    return ids, table


def ill_conditioned(groups):
    """4096 rows of 1e9 + k % 7, in one group or in 7 (group = k % 7 would make every group constant: the groups are k // 7 % 7)"""
    values = [1.0e9 + (k % 7) for k in range(4096)]
    gids = [0] * 4096 if groups == 1 else [k // 7 % 7 for k in range(4096)]
    return batch(values, gids, groups)
