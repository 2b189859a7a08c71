"""Plain-Python restatement of the reference's CovarianceAccumulator, CorrelationAccumulator and RegrAccumulator (physical-expr/src/aggregate/covariance.rs:225-406,
correlation.rs:134-246, regr.rs:228-466) with Python floats (IEEE binary64) in the reference's operation order, grouped the way GroupsAccumulatorAdapter feeds them: every
group has an accumulator of its own that sees its rows in input order, batch by batch.  Argument 0 is `a`, argument 1 is `b`; REGR_*(y, x): a = y, b = x.  Also: exact
rational answers (fractions.Fraction) for every kind, the tolerance of the device tests, and the generators of the random inputs that tests/test_two_argument_aggregates.py runs on
the device and tests/test_comoments_reference.py checks the model on."""
import decimal
import math
from fractions import Fraction

import numpy as np

from moments_reference import GID_NONE, NUMPY_TYPES, VarianceAccumulator, as_f64, first_seen_ids, passes  # noqa: F401  (re-exported to the tests)

COVAR_KINDS = ("COVAR_SAMP", "COVAR_POP")
REGR_KINDS = ("REGR_SLOPE", "REGR_INTERCEPT", "REGR_COUNT", "REGR_R2", "REGR_AVGX", "REGR_AVGY", "REGR_SXX", "REGR_SYY", "REGR_SXY")
KINDS = COVAR_KINDS + ("CORR",) + REGR_KINDS                  # the order of DFGPU_AGG_COVAR_SAMP .. DFGPU_AGG_REGR_SXY (11 .. 22)
KIND_CODES = {k: 11 + i for i, k in enumerate(KINDS)}
STATE_NAMES = {"COVAR": ["count", "mean1", "mean2", "algo_const"], "CORR": ["count", "mean1", "m2_1", "mean2", "m2_2", "algo_const"],
               "REGR": ["count", "mean_x", "mean_y", "m2_x", "m2_y", "algo_const"]}


def family(kind):
    return "COVAR" if kind in COVAR_KINDS else "CORR" if kind == "CORR" else "REGR"


class CovarianceAccumulator:
    def __init__(self):
        self.algo_const, self.mean1, self.mean2, self.count = 0.0, 0.0, 0.0, 0            # covariance.rs:235-243

    def update_batch(self, values1, values2, dtypes=("float64", "float64")):              # :272-311
        for v1, v2 in zip(values1, values2):
            if v1 is None or v2 is None:
                continue
            value1, value2 = as_f64(v1, dtypes[0]), as_f64(v2, dtypes[1])
            new_count = self.count + 1
            delta1 = value1 - self.mean1
            new_mean1 = delta1 / float(new_count) + self.mean1
            delta2 = value2 - self.mean2
            new_mean2 = delta2 / float(new_count) + self.mean2
            new_c = delta1 * (value2 - new_mean2) + self.algo_const
            self.count += 1
            self.mean1 = new_mean1
            self.mean2 = new_mean2
            self.algo_const = new_c

    def merge_batch(self, counts, means1, means2, cs):                                      # :354-382
        for c, m1, m2, cc in zip(counts, means1, means2, cs):
            if c == 0:
                continue
            new_count = self.count + c
            new_mean1 = self.mean1 * float(self.count) / float(new_count) + m1 * float(c) / float(new_count)
            new_mean2 = self.mean2 * float(self.count) / float(new_count) + m2 * float(c) / float(new_count)
            delta1 = self.mean1 - m1
            delta2 = self.mean2 - m2
            new_c = self.algo_const + cc + delta1 * delta2 * float(self.count) * float(c) / float(new_count)
            self.count = new_count
            self.mean1 = new_mean1
            self.mean2 = new_mean2
            self.algo_const = new_c

    def state(self):                                                                        # :263-270
        return (self.count, self.mean1, self.mean2, self.algo_const)

    def evaluate(self, kind):                                                               # :384-401
        count = self.count if kind == "COVAR_POP" else (self.count - 1 if self.count > 0 else self.count)
        return None if count == 0 else self.algo_const / float(count)


class CorrelationAccumulator:
    def __init__(self):
        self.covar, self.stddev1, self.stddev2 = CovarianceAccumulator(), VarianceAccumulator(), VarianceAccumulator()        # correlation.rs:142-148, all Population

    def update_batch(self, values1, values2, dtypes=("float64", "float64")):              # :163-183: the children see the pairs without a NULL
        pairs = [(v1, v2) for v1, v2 in zip(values1, values2) if v1 is not None and v2 is not None]
        v1, v2 = [p[0] for p in pairs], [p[1] for p in pairs]
        self.covar.update_batch(v1, v2, dtypes)
        self.stddev1.update_batch(v1, dtypes[0])
        self.stddev2.update_batch(v2, dtypes[1])

    def merge_batch(self, counts, means1, m2s1, means2, m2s2, cs):                          # :202-216
        self.covar.merge_batch(counts, means1, means2, cs)
        self.stddev1.merge_batch(counts, means1, m2s1)
        self.stddev2.merge_batch(counts, means2, m2s2)

    def state(self):                                                                        # :152-161
        return (self.covar.count, self.covar.mean1, self.stddev1.m2, self.covar.mean2, self.stddev2.m2, self.covar.algo_const)

    def evaluate(self, kind="CORR"):                                                        # :218-236
        c, s1, s2 = self.covar.evaluate("COVAR_POP"), self.stddev1.evaluate("STDDEV_POP"), self.stddev2.evaluate("STDDEV_POP")
        if c is None or s1 is None or s2 is None:
            return None
        return 0.0 if s1 == 0.0 or s2 == 0.0 else c / s1 / s2


def fdiv(a, b):
    """f64 division: IEEE answers where Python raises"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float("nan")
    return math.copysign(float("inf"), a) * math.copysign(1.0, b)


class RegrAccumulator:
    def __init__(self):
        self.count, self.mean_x, self.mean_y, self.m2_x, self.m2_y, self.algo_const = 0, 0.0, 0.0, 0.0, 0.0, 0.0      # regr.rs:240-250

    def update_batch(self, values_y, values_x, dtypes=("float64", "float64")):            # :265-306
        for vy, vx in zip(values_y, values_x):
            if vy is None or vx is None:
                continue
            value_y, value_x = as_f64(vy, dtypes[0]), as_f64(vx, dtypes[1])
            self.count += 1
            delta_x = value_x - self.mean_x
            delta_y = value_y - self.mean_y
            self.mean_x += delta_x / float(self.count)
            self.mean_y += delta_y / float(self.count)
            delta_x_2 = value_x - self.mean_x
            delta_y_2 = value_y - self.mean_y
            self.m2_x += delta_x * delta_x_2
            self.m2_y += delta_y * delta_y_2
            self.algo_const += delta_x * (value_y - self.mean_y)

    def merge_batch(self, counts, means_x, means_y, m2s_x, m2s_y, cs):                      # :359-419
        for count_b, mean_x_b, mean_y_b, m2_x_b, m2_y_b, algo_const_b in zip(counts, means_x, means_y, m2s_x, m2s_y, cs):
            if count_b == 0:
                continue
            count_ab = self.count + count_b
            count_a, count_b = float(self.count), float(count_b)
            d_x = mean_x_b - self.mean_x
            d_y = mean_y_b - self.mean_y
            mean_x_ab = self.mean_x + d_x * count_b / float(count_ab)
            mean_y_ab = self.mean_y + d_y * count_b / float(count_ab)
            m2_x_ab = self.m2_x + m2_x_b + d_x * d_x * count_a * count_b / float(count_ab)
            m2_y_ab = self.m2_y + m2_y_b + d_y * d_y * count_a * count_b / float(count_ab)
            algo_const_ab = self.algo_const + algo_const_b + d_x * d_y * count_a * count_b / float(count_ab)
            self.count, self.mean_x, self.mean_y, self.m2_x, self.m2_y, self.algo_const = count_ab, mean_x_ab, mean_y_ab, m2_x_ab, m2_y_ab, algo_const_ab

    def state(self):                                                                        # :254-262
        return (self.count, self.mean_x, self.mean_y, self.m2_x, self.m2_y, self.algo_const)

    def evaluate(self, kind):                                                               # :420-460
        n = float(self.count)
        cov_pop_x_y, var_pop_x, var_pop_y = fdiv(self.algo_const, n), fdiv(self.m2_x, n), fdiv(self.m2_y, n)

        def nullif_or_stat(cond, stat):
            return None if cond else stat()
        if kind == "REGR_SLOPE":
            return nullif_or_stat(self.count <= 1 or var_pop_x == 0.0, lambda: fdiv(cov_pop_x_y, var_pop_x))
        if kind == "REGR_INTERCEPT":
            return nullif_or_stat(self.count <= 1 or var_pop_x == 0.0, lambda: self.mean_y - fdiv(cov_pop_x_y, var_pop_x) * self.mean_x)
        if kind == "REGR_COUNT":
            return n
        if kind == "REGR_R2":
            return nullif_or_stat(self.count <= 1 or var_pop_x == 0.0 or var_pop_y == 0.0, lambda: fdiv(cov_pop_x_y * cov_pop_x_y, var_pop_x * var_pop_y))
        return nullif_or_stat(self.count < 1, lambda: {"REGR_AVGX": self.mean_x, "REGR_AVGY": self.mean_y, "REGR_SXX": self.m2_x, "REGR_SYY": self.m2_y, "REGR_SXY": self.algo_const}[kind])


ACCUMULATORS = {"COVAR": CovarianceAccumulator, "CORR": CorrelationAccumulator, "REGR": RegrAccumulator}


class GroupedCoMoments:
    """GroupsAccumulatorAdapter over the accumulator of `kind`'s family: one accumulator per group"""

    def __init__(self, kind, dtypes=("float64", "float64")):
        self.kind, self.family, self.dtypes, self.accs = kind, family(kind), tuple(dtypes), []

    def _grow(self, total):
        while len(self.accs) < total:
            self.accs.append(ACCUMULATORS[self.family]())

    def update_batch(self, a, b, gids, opt_filter, total):
        self._grow(total)
        for i, (va, vb, g) in enumerate(zip(a, b, gids)):
            if passes(g, i, opt_filter):
                self.accs[g].update_batch([va], [vb], self.dtypes)

    def merge_batch(self, states, gids, opt_filter, total):
        self._grow(total)
        for i, g in enumerate(gids):
            if passes(g, i, opt_filter):
                self.accs[g].merge_batch(*[[col[i]] for col in states])

    def state(self):
        """the state columns of the family, in the reference's order"""
        rows = [a.state() for a in self.accs]
        return [[r[k] for r in rows] for k in range(len(STATE_NAMES[self.family]))]

    def evaluate(self, kind=None):
        kind = kind or self.kind
        assert family(kind) == self.family
        return [a.evaluate(kind) for a in self.accs]


def model_of(kind, batches, dtypes=("float64", "float64")):
    m = GroupedCoMoments(kind, dtypes)
    for b in batches:
        m.update_batch(b["a"], b["b"], b["gids"], b["filter"], b["total"])
    return m


# ------------------------------------------------------------------ exact arithmetic
def group_pairs(batches, dtypes=("float64", "float64")):
    """the pairs every group receives from update batches, as exact Fractions of their `as f64` casts"""
    total = max([b["total"] for b in batches] + [0])
    out = [[] for _ in range(total)]
    for bt in batches:
        for i, (va, vb, g) in enumerate(zip(bt["a"], bt["b"], bt["gids"])):
            if va is not None and vb is not None and passes(g, i, bt.get("filter")):
                out[g].append((Fraction(as_f64(va, dtypes[0])), Fraction(as_f64(vb, dtypes[1]))))
    return out


def exact_state(pairs):
    """(count, mean_a, mean_b, m2_a, m2_b, c_ab) of exact pairs, as Fractions"""
    n = len(pairs)
    if n == 0:
        return (0,) + (Fraction(0),) * 5
    sa, sb = sum((p[0] for p in pairs), Fraction(0)), sum((p[1] for p in pairs), Fraction(0))
    return (n, sa / n, sb / n, sum((p[0] * p[0] for p in pairs), Fraction(0)) - sa * sa / n, sum((p[1] * p[1] for p in pairs), Fraction(0)) - sb * sb / n,
            sum((p[0] * p[1] for p in pairs), Fraction(0)) - sa * sb / n)


def _dec(fr):
    return decimal.Decimal(fr.numerator) / decimal.Decimal(fr.denominator)


def exact_evaluate(kind, pairs):
    """None where the reference answers NULL, else the exact answer as a decimal.Decimal of 60 digits (x = b, y = a for REGR_*)"""
    n, mean_a, mean_b, m2_a, m2_b, c_ab = exact_state(pairs)
    with decimal.localcontext() as c:
        c.prec = 60
        if kind == "COVAR_POP":
            return None if n == 0 else _dec(c_ab / n)
        if kind == "COVAR_SAMP":
            return None if n <= 1 else _dec(c_ab / (n - 1))
        if kind == "CORR":
            if n == 0:
                return None
            return decimal.Decimal(0) if m2_a == 0 or m2_b == 0 else _dec(c_ab) / (_dec(m2_a) * _dec(m2_b)).sqrt()
        if kind == "REGR_COUNT":
            return decimal.Decimal(n)
        if kind in ("REGR_SLOPE", "REGR_INTERCEPT"):
            return None if n <= 1 or m2_b == 0 else _dec(c_ab / m2_b if kind == "REGR_SLOPE" else mean_a - c_ab / m2_b * mean_b)
        if kind == "REGR_R2":
            return None if n <= 1 or m2_b == 0 or m2_a == 0 else _dec(c_ab * c_ab / (m2_a * m2_b))
        return None if n < 1 else _dec({"REGR_AVGX": mean_b, "REGR_AVGY": mean_a, "REGR_SXX": m2_b, "REGR_SYY": m2_a, "REGR_SXY": c_ab}[kind])


# ------------------------------------------------------------------ the tolerance of the device tests
def scales(batches, dtypes=("float64", "float64")):
    """the largest finite |value| of each argument"""
    out = []
    for key, dt in zip(("a", "b"), dtypes):
        vs = [abs(as_f64(v, dt)) for b in batches for v in b[key] if v is not None]
        out.append(max([v for v in vs if math.isfinite(v)] + [0.0]))
    return tuple(out)


def value_floor(kind, scale_a, scale_b):
    """The absolute floor beside 1e-9 relative for a result of `kind` over arguments of these scales.  c_ab, SXY and COVAR carry the unit a * b, the m2s the square of
    their argument's unit, the means their argument's: 1e-9 of that unit.  CORR and R2 lie in [-1, 1]: 1e-9.  SLOPE is c_ab / m2_x, a quantity of the unit y / x, and
    INTERCEPT = mean_y - slope * mean_x one of the unit y: 1e-9 of those (the inputs' spread is comparable to their scale, so m2_x is not small against scale_x^2)."""
    sy, sx = scale_a, scale_b
    return 1e-9 * {"COVAR_SAMP": sx * sy, "COVAR_POP": sx * sy, "CORR": 1.0, "REGR_SLOPE": sy / sx if sx else 0.0, "REGR_INTERCEPT": sy, "REGR_COUNT": 0.0, "REGR_R2": 1.0,
                   "REGR_AVGX": sx, "REGR_AVGY": sy, "REGR_SXX": sx * sx, "REGR_SYY": sy * sy, "REGR_SXY": sx * sy}[kind]


def state_floors(fam, scale_a, scale_b):
    """value_floor's reasoning for the state columns of a family, in their order"""
    by_name = {"count": 0.0, "mean1": scale_a, "mean2": scale_b, "m2_1": scale_a ** 2, "m2_2": scale_b ** 2, "mean_x": scale_b, "mean_y": scale_a, "m2_x": scale_b ** 2,
               "m2_y": scale_a ** 2, "algo_const": scale_a * scale_b}
    return [1e-9 * by_name[n] for n in STATE_NAMES[fam]]


def close(got, want, floor=0.0):
    return abs(got - want) <= max(1e-9 * abs(want), floor)


# ------------------------------------------------------------------ the random inputs of the device tests
COMOMENTS_LDS_GROUPS = 1024        # T: the largest number of groups the LDS path of csrc/comoments.hip takes (COMOMENTS_LDS_GROUPS there)
COMOMENTS_LDS_SMALL = 512          # up to here that path runs with its smaller LDS arrays (COMOMENTS_LDS_SMALL there)
PATH_ROWS = (0, 1, 63, 64, 65, 255, 256, 257)          # wave and workgroup (256 lanes) edges
PATH_TOTALS = (1, 2, COMOMENTS_LDS_SMALL, COMOMENTS_LDS_SMALL + 1, COMOMENTS_LDS_GROUPS, COMOMENTS_LDS_GROUPS + 1)


def batch(a, b, gids, total, opt_filter=None):
    return {"a": list(a), "b": list(b), "gids": [int(g) for g in gids], "filter": opt_filter, "total": int(total)}


def correlated_pairs(rng, gids, total):
    """Group g draws b from N(mb_g, 3^2) and a = ma_g + r_g * (b - mb_g) + N(0, 3^2), with ma_g, mb_g uniform in [-10, 10] and r_g in [-2, 2]: the spread (sd >= 3) is
    comparable to the scale (|value| <= ~30), every correlation from strongly negative to strongly positive occurs, and no group is constant"""
    t = max(total, 1)
    ma, mb, r = rng.uniform(-10.0, 10.0, t), rng.uniform(-10.0, 10.0, t), rng.uniform(-2.0, 2.0, t)
    g = np.minimum(np.asarray(gids, dtype=np.int64), t - 1)
    db = 3.0 * rng.standard_normal(len(g))
    return (ma[g] + r[g] * db + 3.0 * rng.standard_normal(len(g))).tolist(), (mb[g] + db).tolist()


def path_batch(n, total, ids="random"):
    """one update batch of n rows over `total` groups: random ids (some groups get no row), all-equal ids (every wave uniform) or strictly alternating ids (no wave uniform)"""
    rng = np.random.default_rng(2000 * n + total + {"random": 0, "equal": 7, "alternating": 13}[ids])
    if ids == "random":
        gids = rng.integers(0, total, n)
    elif ids == "equal":
        gids = np.full(n, total - 1)
    else:
        gids = np.arange(n) % 2 * (total - 1)
    a, b = correlated_pairs(rng, gids, total)
    return batch(a, b, gids, total)


def ragged_batches(total, seed=3):
    """a few thousand rows in three ragged batches over `total` groups (for total = 1 and 2 every group is hit in every batch)"""
    rng = np.random.default_rng(seed + total)
    out = []
    for n in (1237, 2049, 811):
        gids = rng.integers(0, total, n)
        a, b = correlated_pairs(rng, gids, total)
        out.append(batch(a, b, gids, total))
    return out


def nulls_filters_batch(n=1500, total=37, seed=21, all_null_group=True):
    """NULLs in a alone (15 %), in b alone (15 %) and in both (10 %), a filter with false and NULL entries, ids of 0xFFFFFFFF; the rows of group 0 are NULL in one
    argument or the other throughout"""
    rng = np.random.default_rng(seed)
    gids = rng.integers(0, total, n)
    a, b = correlated_pairs(rng, gids, total)
    for i, r in enumerate(rng.random(n)):
        if r < 0.15 or 0.3 <= r < 0.4 or (all_null_group and gids[i] == 0 and i % 2 == 0):
            a[i] = None
        if 0.15 <= r < 0.4 or (all_null_group and gids[i] == 0 and i % 2 == 1):
            b[i] = None
    filt = [[True, True, True, False, None][k] for k in rng.integers(0, 5, n)]
    gids = [GID_NONE if r < 0.1 else int(g) for g, r in zip(gids, rng.random(n))]
    return batch(a, b, gids, total, filt)


def growing_batches(seed=33):
    """new groups appear in batches 2 and 3 and the total grows across COMOMENTS_LDS_GROUPS"""
    rng = np.random.default_rng(seed)
    out = []
    for n, total in ((300, 5), (700, 11), (4000, COMOMENTS_LDS_GROUPS + 76)):
        gids = rng.integers(0, total, n)
        a, b = correlated_pairs(rng, gids, total)
        out.append(batch(a, b, gids, total))
    return out


def merge_inputs(total=300, seed=44):
    """the update batches of two accumulators whose states are merged into a third"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (2500, 1700):
        gids = rng.integers(0, total, n)
        a, b = correlated_pairs(rng, gids, total)
        out.append(batch([None if r < 0.1 else v for v, r in zip(a, rng.random(n))], b, gids, total))
    return out


TYPE_PAIRS = (("int32", "float64"), ("uint64", "float32"), ("int8", "int8"))


def typed_values(rng, dtype, gids, total):
    if dtype.startswith("float"):
        return [NUMPY_TYPES[dtype](v).item() for v in correlated_pairs(rng, gids, total)[0]]
    info = np.iinfo(NUMPY_TYPES[dtype])
    return [int(v) for v in rng.integers(info.min, info.max, len(gids), dtype=NUMPY_TYPES[dtype], endpoint=True)]


def typed_batch(dtypes, n=600, total=13, seed=55):
    """each argument of its own type over that type's whole range (UInt64: above 2^63 too; floats: normal around a per-group mean)"""
    rng = np.random.default_rng(seed + sum(ord(c) for c in dtypes[0] + dtypes[1]))
    gids = rng.integers(0, total, n)
    return batch(typed_values(rng, dtypes[0], gids, total), typed_values(rng, dtypes[1], gids, total), gids, total)


CONSTANT = 0.1                     # 0.1 + 0.1 + 0.1 != 0.3: a sum-then-divide mean of it is not 0.1 for most counts


def constant_batches(total, seed=71, batches=3, rows=700):
    """`batches` batches of `rows` rows over `total` groups.  Group 0: a is 0.1 in every row; group 1: b is 0.1 in every row; group 2 (total >= 4): both are; every other
    group varies in both.  Every group has one row per batch and `rows` more rows go to the first eight groups at random (some 90 per batch to each constant group), shuffled."""
    rng = np.random.default_rng(seed + total)
    out = []
    for _ in range(batches):
        gids = np.concatenate([np.arange(total), rng.integers(0, min(total, 8), rows)])
        rng.shuffle(gids)
        a, b = correlated_pairs(rng, gids, total)
        for i, g in enumerate(gids):
            if g == 0 or (g == 2 and total >= 4):
                a[i] = CONSTANT
            if g == 1 or (g == 2 and total >= 4):
                b[i] = CONSTANT
        out.append(batch(a, b, gids, total))
    return out


def plan_tables(seed=5, batches=3, rows=4000, groups=40):
    """the plan-level input: per batch the columns k (Int64 key, 5 % NULL), y and x (Float64 multiples of 1/64, 15 % NULL each), v (Int32, no NULL), f (Boolean FILTER
    column with false and NULL entries), w (Float64, x where x is large enough for the FilterExec `w > -5` to keep most rows, never NULL)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batches):
        k = rng.integers(0, groups, rows)
        y, x = correlated_pairs(rng, k, groups)
        y, x = [round(v * 64.0) / 64.0 for v in y], [round(v * 64.0) / 64.0 for v in x]            # multiples of 1/64: their Float64 SUM is exact in any order
        out.append({"k": [None if r < 0.05 else int(v) for v, r in zip(k, rng.random(rows))],
                    "y": [None if r < 0.15 else v for v, r in zip(y, rng.random(rows))],
                    "x": [None if r < 0.15 else v for v, r in zip(x, rng.random(rows))],
                    "v": [int(v) for v in rng.integers(-1000, 1000, rows)],
                    "f": [[True, True, False, None][j] for j in rng.integers(0, 4, rows)],
                    "w": list(x)})
    return out
