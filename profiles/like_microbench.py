"""Device time of LIKE (dfgpu_like) over an o_comment-shaped column, next to code that also reads every string byte: dfgpu_hash_columns, one lane per row.

    python profiles/like_microbench.py [--rows 100000000] [--runs 25] [--out profiles/like_microbench.json]

--rows rows of 19 to 78 random lower-case bytes, generated on the device; 3 % of the rows each hold `special` .. `requests`, `green`, a leading `PROMO` and
a trailing `BRASS`.  Utf8 offsets are 32 bits wide, so the column is cut into batches of at most 25 M rows (about 1.2 GB of values each); one figure is the
device time of the call over every batch, measured with the context's device-time spans (dfgpu_span_*) after warm-up, the median of --runs runs.
  special_requests  LIKE '%special%requests%'     k_like_scan + k_like_resolve, two middle segments
  green             LIKE '%green%'                k_like_scan + k_like_resolve, one middle segment
  promo             LIKE 'PROMO%'                 k_like_anchor
  brass             LIKE '%BRASS'                 k_like_anchor
  underscore        LIKE '%gre_n%'                k_like_row: one lane per row walks characters
  hash              dfgpu_hash_columns            the yardstick: one lane per row reads every byte of its string
  dictionary        LIKE '%green%' over --rows Int32 codes into 1 M entries: the pattern once per entry, then k_dict_predicate_i32
  low_entropy       25 M rows over the three characters `a`, `b` and blank: LIKE '%abab%baba%' (k_like_scan: every third byte is a candidate of each
                    segment, so the candidate check against LDS runs in every lane), LIKE '%aba_%baba%' (k_like_row) and the hash yardstick over that column
`bytes` / `gb_per_s`: the input the algorithm needs -- 4 (one offset) + the row's value bytes, 4 for the dictionary arm.  `traffic_bytes` / `traffic_gb_per_s`
add what the chosen kernels move on top of that: the result bits, and for k_like_scan + k_like_resolve one bit per value byte and part written and read back.
Every scalar-pattern call holds one host read-back (offsets[0], offsets[n] and the pattern come back through the mailbox before the kernels are launched); it
lies inside the timed span, once per batch, and the hash yardstick has no such wait.  The string arms alternate inside one process, so they share whatever
else the machine is doing.  The driver starts one child process per step under a time limit of its own and stops at the first
step that fails; it does not touch the device itself."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"strings": 420, "dictionary": 240, "low_entropy": 240}          # seconds
BATCH_ROWS = 25_000_000
PATTERNS = {"special_requests": "%special%requests%", "green": "%green%", "promo": "PROMO%", "brass": "%BRASS", "underscore": "%gre_n%"}
BITMAP_PARTS = {"special_requests": 2, "green": 1, "promo": 0, "brass": 0, "underscore": 0}          # parts k_like_scan writes a bitmap for


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


def stats(v, bytes_total, traffic):
    return {"median_ms": median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / median(v), "bytes": bytes_total,
            "gb_per_s": bytes_total / (median(v) * 1e-3) / 1e9, "traffic_bytes": traffic, "traffic_gb_per_s": traffic / (median(v) * 1e-3) / 1e9}


def like_traffic(n, value_bytes, parts):
    """input + result bits + per bitmap part one bit per value byte written by the scan and read by the resolve pass"""
    return 4 * n + value_bytes + n // 8 + parts * 2 * (value_bytes // 8)


def comment_batch(ctx, n, gen, torch, letters=None):
    """-> (Utf8 array over device tensors, offsets, values); letters: the bytes to draw from (default a..z), no needles then"""
    from dfgpu import capi
    lens = torch.randint(19, 79, (n,), dtype=torch.int64, device="cuda", generator=gen)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    assert total < 2**31 - 16
    if letters is not None:
        table = torch.tensor(list(letters.encode()), dtype=torch.uint8, device="cuda")
        values = table[torch.randint(0, len(table), (total,), device="cuda", generator=gen)]
    else:
        values = torch.randint(97, 123, (total,), dtype=torch.uint8, device="cuda", generator=gen)
    pick = torch.rand(n, device="cuda", generator=gen) if letters is None else torch.ones(n, device="cuda")

    def put(lo, hi, word, at_end=False, shift=0):
        rows = torch.nonzero((pick >= lo) & (pick < hi)).flatten()
        w = torch.tensor(list(word.encode()), dtype=torch.uint8, device="cuda")
        start = (offsets[rows + 1] - len(word)) if at_end else (offsets[rows] + shift)
        values[(start[:, None] + torch.arange(len(word), device="cuda")[None, :]).flatten()] = w.repeat(len(rows))
    put(0.00, 0.03, "special", shift=1); put(0.00, 0.03, "requests", shift=10)
    put(0.03, 0.06, "green", shift=3)
    put(0.06, 0.09, "PROMO")
    put(0.09, 0.12, "BRASS", at_end=True)
    off32 = offsets.to(torch.int32)
    d = capi.ArrayDesc()
    d.type, d.length, d.null_count, d.values, d.offsets, d.values_bytes = capi.UTF8, n, 0, values.data_ptr(), off32.data_ptr(), total
    return ctx.wrap_device(d, keepalive=(values, off32)), off32, values


def step_strings(n, runs):
    import pyarrow as pa
    import torch
    import dfgpu
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from like_reference import like_rows
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    batches, value_bytes = [], 0
    for lo in range(0, n, BATCH_ROWS):
        arr, off32, values = comment_batch(ctx, min(BATCH_ROWS, n - lo), gen, torch)
        batches.append((arr, off32, values))
        value_bytes += int(off32[-1].item())
    torch.cuda.synchronize()
    pats = {k: ctx.from_arrow(pa.array([p], type=pa.utf8())) for k, p in PATTERNS.items()}
    arms = {k: (lambda k=k: [ctx.like(b[0], pats[k]) for b in batches]) for k in PATTERNS}
    arms["hash"] = lambda: [ctx.hash_columns([b[0]]) for b in batches]
    # every pattern once against the checker, on a prefix of the first batch: a wrong kernel is not worth timing
    m = min(len(batches[0][0]), 200_000)
    off = batches[0][1][: m + 1].cpu().numpy()
    raw = batches[0][2][: int(off[-1])].cpu().numpy().tobytes()
    rows = [raw[off[i]:off[i + 1]].decode() for i in range(m)]
    selectivity = {}
    for k, p in PATTERNS.items():
        got = ctx.like(batches[0][0].slice(0, m), pats[k]).to_arrow().to_pylist()
        assert got == like_rows(rows, p), f"{k}: wrong result"
        selectivity[k] = sum(got) / m
    ms = {k: [] for k in arms}
    for r in range(5 + runs):
        for k in arms:
            t = timed(ctx, arms[k])
            if r >= 5:
                ms[k].append(t)
    total = 4 * n + value_bytes
    out = {k: dict(stats(v, total, like_traffic(n, value_bytes, BITMAP_PARTS[k]) if k in PATTERNS else total + 8 * n),
                   **({"selectivity": selectivity[k], "pattern": PATTERNS[k]} if k in PATTERNS else {})) for k, v in ms.items()}
    print(json.dumps({"step": "strings", "rows": n, "runs": runs, "value_bytes": value_bytes, "batches": len(batches), "arms": out}), flush=True)


def step_dictionary(n, runs):
    import numpy as np
    import pyarrow as pa
    import torch
    import dfgpu
    from dfgpu import capi
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(13)
    entries = 1_000_000
    urls, off32, values = comment_batch(ctx, entries, gen, torch)
    codes = torch.randint(0, entries, (n,), dtype=torch.int32, device="cuda", generator=gen)
    torch.cuda.synchronize()
    dd, d = capi.ArrayDesc(), capi.ArrayDesc()
    dd.type, dd.length, dd.null_count, dd.values, dd.offsets, dd.values_bytes = capi.UTF8, entries, 0, values.data_ptr(), off32.data_ptr(), int(off32[-1].item())
    d.type, d.key_type, d.length, d.null_count, d.values = capi.DICTIONARY, capi.INT32, n, 0, codes.data_ptr()
    import ctypes as C
    d.dictionary = C.pointer(dd)
    col = ctx.wrap_device(d, keepalive=(codes, values, off32))
    pat = ctx.from_arrow(pa.array(["%green%"], type=pa.utf8()))
    m = min(n, 1 << 20)
    per_entry = np.asarray(ctx.like(urls, pat).to_arrow())
    got = np.asarray(ctx.like(col, pat).slice(0, m).to_arrow())
    assert np.array_equal(got, per_entry[codes[:m].cpu().numpy()]), "dictionary: wrong result"
    ms = []
    for r in range(5 + runs):
        t = timed(ctx, lambda: ctx.like(col, pat))
        if r >= 5:
            ms.append(t)
    entry_bytes = int(off32[-1].item())
    out = {"dictionary": dict(stats(ms, 4 * n, 4 * n + n // 8 + like_traffic(entries, entry_bytes, 1)), entries=entries, pattern="%green%")}
    print(json.dumps({"step": "dictionary", "rows": n, "runs": runs, "arms": out}), flush=True)


def step_low_entropy(n, runs):
    import pyarrow as pa
    import torch
    import dfgpu
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from like_reference import like_rows
    ctx = dfgpu.Context(0)
    n = min(n, BATCH_ROWS)
    gen = torch.Generator(device="cuda").manual_seed(17)
    col, off32, values = comment_batch(ctx, n, gen, torch, letters="ab ")
    torch.cuda.synchronize()
    value_bytes = int(off32[-1].item())
    pats = {"low_entropy_scan": "%abab%baba%", "low_entropy_row": "%aba_%baba%"}
    dev = {k: ctx.from_arrow(pa.array([p], type=pa.utf8())) for k, p in pats.items()}
    m = min(n, 100_000)
    off = off32[: m + 1].cpu().numpy()
    raw = values[: int(off[-1])].cpu().numpy().tobytes()
    rows = [raw[off[i]:off[i + 1]].decode() for i in range(m)]
    for k, p in pats.items():
        assert ctx.like(col.slice(0, m), dev[k]).to_arrow().to_pylist() == like_rows(rows, p), f"{k}: wrong result"
    arms = {k: (lambda k=k: ctx.like(col, dev[k])) for k in pats}
    arms["low_entropy_hash"] = lambda: ctx.hash_columns([col])
    ms = {k: [] for k in arms}
    for r in range(5 + runs):
        for k in arms:
            t = timed(ctx, arms[k])
            if r >= 5:
                ms[k].append(t)
    total = 4 * n + value_bytes
    traffic = {"low_entropy_scan": like_traffic(n, value_bytes, 2), "low_entropy_row": like_traffic(n, value_bytes, 0), "low_entropy_hash": total + 8 * n}
    out = {k: dict(stats(v, total, traffic[k]), rows=n, **({"pattern": pats[k]} if k in pats else {})) for k, v in ms.items()}
    print(json.dumps({"step": "low_entropy", "rows": n, "runs": runs, "arms": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "like_microbench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs: at least 20")
    if a.step:
        return {"strings": step_strings, "dictionary": step_dictionary, "low_entropy": step_low_entropy}[a.step](a.rows, a.runs)
    res = {"rows": a.rows, "runs": a.runs, "arms": {}}
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--rows", str(a.rows), "--runs", str(a.runs)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"step {name} failed with exit status {r.returncode}: stopping")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        res["arms"].update(line["arms"])
        for k in ("value_bytes", "batches"):
            if k in line:
                res[k] = line[k]
    h = res["arms"]["hash"]
    res["hash_spread"] = h["spread"]
    res["green_over_hash"] = res["arms"]["green"]["median_ms"] / h["median_ms"]
    res["green_over_underscore"] = res["arms"]["green"]["median_ms"] / res["arms"]["underscore"]["median_ms"]
    res["low_entropy_scan_over_hash"] = res["arms"]["low_entropy_scan"]["median_ms"] / res["arms"]["low_entropy_hash"]["median_ms"]
    res["low_entropy_scan_over_row"] = res["arms"]["low_entropy_scan"]["median_ms"] / res["arms"]["low_entropy_row"]["median_ms"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
