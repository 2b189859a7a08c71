"""Device time of the CASE select kernel (dfgpu_case -> k_case_select) next to a kernel of the same traffic that it does not share code with.

    python profiles/case_microbench.py [--rows 100000000] [--runs 25] [--out profiles/case_microbench.json]

Float64 columns of --rows rows (800 MB each at the default: well past the 256 MB Infinity Cache), generated on the device.  Timed with the context's
device-time spans (dfgpu_span_*) after warm-up; every figure is the median of --runs runs.
  a  dfgpu_case, one WHEN bitmap, THEN and ELSE columns        24 B + 1 bit per row
  b  the same with scalar THEN and ELSE                         8 B + 1 bit per row
  c  as a, the WHEN true only in every 16th 64-row group        nominally as a; a group that is all one branch fetches that operand alone (16 B + 1 bit)
  d  dfgpu_binary Float64 column + column (k_arith)             24 B per row: the yardstick
a and d alternate inside one process.  The driver starts one child process per step under a time limit of its own and stops at the first step that fails; it
does not touch the device itself."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"a+d": 240, "b": 180, "c": 180}          # seconds


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


def step(name, n, runs):
    import numpy as np
    import pyarrow as pa
    import torch
    import dfgpu
    from dfgpu import capi
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    y = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    words = (n + 63) // 64
    if name == "c":
        w = torch.zeros(words, dtype=torch.int64, device="cuda")
        w[::16] = -1
        bits = w.view(torch.uint8)
    else:
        bits = torch.randint(0, 256, (words * 8,), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    X, Y, W = ctx.wrap_tensor(x, capi.FLOAT64), ctx.wrap_tensor(y, capi.FLOAT64), ctx.wrap_tensor_bool(bits, n)
    sx, sy = ctx.from_arrow(pa.array([1.5])), ctx.from_arrow(pa.array([-2.5]))
    arms = {"a": (lambda: ctx.case([W], [X], Y), 24 + 1 / 8), "c": (lambda: ctx.case([W], [X], Y), 24 + 1 / 8),
            "b": (lambda: ctx.case([W], [sx], sy, then_scalar=[True], else_scalar=True), 8 + 1 / 8),
            "d": (lambda: ctx.binary(capi.OP_ADD, X, Y), 24)}
    # the result once against torch, on a prefix: a wrong kernel is not worth timing
    m = min(n, 1 << 20)
    sel = ((bits[: (m + 7) // 8].cpu().numpy()[:, None] >> np.arange(8)) & 1).reshape(-1)[:m].astype(bool)
    for arm in name.split("+"):
        got = arms[arm][0]().slice(0, m).to_numpy()
        want = {"a": np.where(sel, x[:m].cpu().numpy(), y[:m].cpu().numpy()), "b": np.where(sel, 1.5, -2.5), "d": (x[:m] + y[:m]).cpu().numpy()}["a" if arm == "c" else arm]
        assert np.array_equal(got, want), f"arm {arm}: wrong result"
    ms = {arm: [] for arm in name.split("+")}
    for r in range(5 + runs):
        for arm in ms:
            t = timed(ctx, arms[arm][0])
            if r >= 5:
                ms[arm].append(t)
    out = {arm: {"median_ms": median(v), "min_ms": min(v), "max_ms": max(v), "bytes_per_row": arms[arm][1], "gb_per_s": arms[arm][1] * n / (median(v) * 1e-3) / 1e9} for arm, v in ms.items()}
    print(json.dumps({"step": name, "rows": n, "runs": runs, "arms": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "case_microbench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if a.step:
        return step(a.step, a.rows, a.runs)
    arms = {}
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--rows", str(a.rows), "--runs", str(a.runs)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"step {name} failed with exit status {r.returncode}: stopping")
        arms.update(json.loads(r.stdout.strip().splitlines()[-1])["arms"])
    res = {"rows": a.rows, "runs": a.runs, "arms": arms, "a_over_d": arms["a"]["median_ms"] / arms["d"]["median_ms"], "c_over_a": arms["c"]["median_ms"] / arms["a"]["median_ms"]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
