"""Device time of date_part('minute') and date_trunc('minute') over a Timestamp column next to a cast that moves the same bytes.

    python profiles/timestamp_microbench.py [--rows 100000000] [--runs 25] [--out profiles/timestamp_microbench.json]

Per unit (second, millisecond, microsecond, nanosecond) one child process under a time limit of its own times three calls over the same --rows instants, far
more than the caches hold: date_part('minute', ts) (k_ts_part: 8 B in, 8 B out per row), date_trunc('minute', ts) (k_ts_trunc: the same bytes, plus the
read-back of its error flag) and dfgpu_cast Int64 -> Float64 over the same buffer (k_cast: the same bytes, and a flag read-back too).  A figure is the device
time of the call measured with the context's device-time spans (dfgpu_span_*) after warm-up: the median of --runs runs with minimum, maximum and spread; the
arms alternate inside the process, so they share whatever else the machine is doing.  `part_over_cast` and `trunc_over_cast` are ratios of the medians.
The driver stops at the first step that fails and does not touch the device itself."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNITS = {"s": (16, 1), "ms": (17, 10**3), "us": (18, 10**6), "ns": (19, 10**9)}          # DFGPU_TIMESTAMP_* and units per second
STEP_SECONDS = 180
FN_DATE_PART, FN_DATE_TRUNC = 1, 7


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def timed(ctx, fn):
    import ctypes as C
    span, ns = C.c_int64(), C.c_int64()
    ctx.check(ctx.lib.dfgpu_span_begin(ctx.h, C.byref(span)))
    out = fn()
    ctx.check(ctx.lib.dfgpu_span_end(ctx.h, span))
    ctx.check(ctx.lib.dfgpu_span_elapsed_ns(ctx.h, span, C.byref(ns)))
    del out
    return ns.value / 1e6


def stats(v, bytes_total):
    return {"median_ms": median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / median(v), "bytes": bytes_total,
            "gb_per_s": bytes_total / (median(v) * 1e-3) / 1e9}


def step(unit, n, runs):
    import numpy as np
    import pyarrow as pa
    import torch
    import dfgpu
    from dfgpu import capi
    code, per_sec = UNITS[unit]
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(19)
    # 2013-07-01 .. 2013-07-31 at the unit's resolution (ClickBench's EventTime month)
    secs = torch.randint(1372636800, 1375315200, (n,), dtype=torch.int64, device="cuda", generator=gen)
    sub = torch.randint(0, per_sec, (n,), dtype=torch.int64, device="cuda", generator=gen)
    vals = secs * per_sec + sub
    del secs, sub
    torch.cuda.synchronize()
    ts, ints = ctx.wrap_tensor(vals, code), ctx.wrap_tensor(vals, capi.INT64)
    minute = ctx.from_arrow(pa.array(["minute"], type=pa.utf8()))
    m = min(n, 1 << 20)
    host = vals[:m].cpu().numpy()
    got = np.asarray(ctx.scalar_function(FN_DATE_PART, [minute, ts.slice(0, m)], [True, False]).to_arrow())
    assert np.array_equal(got, (host // per_sec % 3600 // 60).astype(np.float64)), "date_part minute: wrong result"
    got = ctx.scalar_function(FN_DATE_TRUNC, [minute, ts.slice(0, m)], [True, False]).to_arrow().cast(pa.int64()).to_numpy()
    assert np.array_equal(got, host // (60 * per_sec) * (60 * per_sec)), "date_trunc minute: wrong result"
    arms = {"date_part_minute": lambda: ctx.scalar_function(FN_DATE_PART, [minute, ts], [True, False]),
            "date_trunc_minute": lambda: ctx.scalar_function(FN_DATE_TRUNC, [minute, ts], [True, False]),
            "cast_int64_float64": lambda: ctx.cast(ints, capi.FLOAT64)}
    ms = {k: [] for k in arms}
    for r in range(5 + runs):
        for k in arms:
            t = timed(ctx, arms[k])
            if r >= 5:
                ms[k].append(t)
    out = {k: stats(v, 16 * n) for k, v in ms.items()}
    print(json.dumps({"unit": unit, "arms": out, "part_over_cast": out["date_part_minute"]["median_ms"] / out["cast_int64_float64"]["median_ms"],
                      "trunc_over_cast": out["date_trunc_minute"]["median_ms"] / out["cast_int64_float64"]["median_ms"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timestamp_microbench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if a.step:
        return step(a.step, a.rows, a.runs)
    res = {"rows": a.rows, "runs": a.runs, "units": {}}
    for unit in UNITS:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", unit, "--rows", str(a.rows), "--runs", str(a.runs)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"unit {unit} failed with exit status {r.returncode}: stopping")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"unit {unit} done", file=sys.stderr, flush=True)
        res["units"][line.pop("unit")] = line
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({u: {"part_over_cast": v["part_over_cast"], "trunc_over_cast": v["trunc_over_cast"]} for u, v in res["units"].items()}))


if __name__ == "__main__":
    main()
