"""Device time of the scalar functions (dfgpu_scalar_function) next to calls that move the same bytes.

    python profiles/scalar_fn_microbench.py [--rows 100000000] [--runs 25] [--out profiles/scalar_fn_microbench.json]

One figure is the device time of the call over the whole column (Utf8 offsets are 32 bits wide, so string columns are cut into batches of at most 25 M rows),
measured with the context's device-time spans (dfgpu_span_*) after warm-up: the median of --runs runs, with minimum, maximum and spread.  The arms of a step
alternate inside one process, so they share whatever else the machine is doing.
  dates       date_part('year', d) over --rows Date32 rows (k_date_part: 4 B in, 8 B out per row) next to dfgpu_cast Int32 -> Float64 over the same buffer
              (k_cast: the same bytes); `year_over_cast` is the ratio of the medians
  strings     character_length over --rows rows of 19 to 78 random bytes, every tenth character a 2-byte one (the LIKE microbenchmark's shape), next to
              dfgpu_hash_columns over the same column, which also reads every string byte once with a lane per row
  dictionary  character_length over --rows Int32 codes into 1 M such entries: once per entry, then k_dict_gather
  phone       substr(s, 1, 2) over --rows rows of 15 bytes (TPC-H Q22's c_phone): the range pass reads each row's offsets and first word only
  crossing    character_length and left(s, -1) (both count every lead byte of the row) over columns of equal-length rows of 32 .. 1024 bytes, 256 MB each, once with
              the lane-per-row and once with the wave-per-row kernels (option string_wave_row_bytes): where the two cross is STR_WAVE_ROW_BYTES.  left(s, 3) and
              left(s, 31) are row prefixes, which read the head of a row only: the library keeps a literal prefix of at most 31 code points on the lane kernel
              whatever the row length, and these arms show both kernels on it
`bytes` is the input and output the algorithm needs; `traffic_bytes` adds what the chosen kernels move on top (lengths, source positions and 64-bit offsets of a
Utf8 result written and read back).  The driver starts one child process per step under a time limit of its own and stops at the first step that fails; it does
not touch the device itself."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"dates": 180, "strings": 300, "dictionary": 180, "phone": 240, "crossing": 300}          # seconds
BATCH_ROWS = 25_000_000
FN_DATE_PART, FN_CHARACTER_LENGTH, FN_SUBSTR, FN_LEFT = 1, 2, 3, 4
CROSSING_ROW_BYTES = [32, 64, 96, 128, 192, 256, 384, 512, 1024]
LEFT_ARMS = {"left_minus_1": -1, "left_3": 3, "left_31": 31}          # left(s, n): all but the last code point (count, skip, copy); a row prefix of 3 and of 31 code points


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


def stats(v, bytes_total, traffic=None):
    traffic = bytes_total if traffic is None else traffic
    return {"median_ms": median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / median(v), "bytes": bytes_total,
            "gb_per_s": bytes_total / (median(v) * 1e-3) / 1e9, "traffic_bytes": traffic, "traffic_gb_per_s": traffic / (median(v) * 1e-3) / 1e9}


def run_arms(ctx, arms, runs):
    ms = {k: [] for k in arms}
    for r in range(5 + runs):
        for k in arms:
            t = timed(ctx, arms[k])
            if r >= 5:
                ms[k].append(t)
    return ms


def wrap_utf8(ctx, values, off32, n, total):
    from dfgpu import capi
    d = capi.ArrayDesc()
    d.type, d.length, d.null_count, d.values, d.offsets, d.values_bytes = capi.UTF8, n, 0, values.data_ptr(), off32.data_ptr(), total
    return ctx.wrap_device(d, keepalive=(values, off32))


def text_batch(ctx, n, gen, torch, lo=19, hi=78):
    """n rows of lo .. hi bytes: lower-case letters, every tenth character U+00E4 (2 bytes, never cut by a row's end) -> (array, offsets, values)"""
    lens = torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device="cuda", generator=gen)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    assert total < 2**31 - 16
    values = torch.randint(97, 123, (total,), dtype=torch.uint8, device="cuda", generator=gen)
    lead = torch.nonzero(torch.rand(total, device="cuda", generator=gen) < 0.1).flatten()
    lead = lead[(lead % 2 == 0) & (lead + 1 < total)]                       # even positions only: no two pairs overlap
    row_of_next = torch.searchsorted(offsets, lead + 1, right=True)
    row_of_lead = torch.searchsorted(offsets, lead, right=True)
    lead = lead[row_of_next == row_of_lead]                                # both bytes in one row
    values[lead] = 0xC3
    values[lead + 1] = 0xA4
    off32 = offsets.to(torch.int32)
    return wrap_utf8(ctx, values, off32, n, total), off32, values


def host_rows(off32, values, m):
    off = off32[: m + 1].cpu().numpy()
    raw = values[: int(off[-1])].cpu().numpy().tobytes()
    return [raw[off[i]:off[i + 1]].decode() for i in range(m)]


def step_dates(n, runs):
    import numpy as np
    import pyarrow as pa
    import torch
    import dfgpu
    from dfgpu import capi
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(3)
    days = torch.randint(8035, 10592, (n,), dtype=torch.int32, device="cuda", generator=gen)          # 1992-01-01 .. 1998-12-31
    torch.cuda.synchronize()
    d, i = capi.ArrayDesc(), capi.ArrayDesc()
    d.type, d.length, d.null_count, d.values = capi.DATE32, n, 0, days.data_ptr()
    i.type, i.length, i.null_count, i.values = capi.INT32, n, 0, days.data_ptr()
    dates, ints = ctx.wrap_device(d, keepalive=(days,)), ctx.wrap_device(i, keepalive=(days,))
    parts = {p: ctx.from_arrow(pa.array([p], type=pa.utf8())) for p in ("year", "week", "epoch")}
    m = min(n, 1 << 20)
    got = np.asarray(ctx.scalar_function(FN_DATE_PART, [parts["year"], dates.slice(0, m)], [True, False]).to_arrow())
    want = (days[:m].cpu().numpy().astype("datetime64[D]").astype("datetime64[Y]").astype(np.int64) + 1970).astype(np.float64)
    assert np.array_equal(got, want), "date_part year: wrong result"
    arms = {f"date_part_{p}": (lambda p=p: ctx.scalar_function(FN_DATE_PART, [parts[p], dates], [True, False])) for p in parts}
    arms["cast_int32_float64"] = lambda: ctx.cast(ints, capi.FLOAT64)
    ms = run_arms(ctx, arms, runs)
    out = {k: stats(v, 12 * n) for k, v in ms.items()}
    print(json.dumps({"step": "dates", "arms": out, "year_over_cast": out["date_part_year"]["median_ms"] / out["cast_int32_float64"]["median_ms"]}), flush=True)


def step_strings(n, runs):
    import torch
    import dfgpu
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    batches, value_bytes = [], 0
    for lo in range(0, n, BATCH_ROWS):
        batches.append(text_batch(ctx, min(BATCH_ROWS, n - lo), gen, torch))
        value_bytes += int(batches[-1][1][-1].item())
    torch.cuda.synchronize()
    m = min(len(batches[0][0]), 200_000)
    rows = host_rows(batches[0][1], batches[0][2], m)
    got = ctx.scalar_function(FN_CHARACTER_LENGTH, [batches[0][0].slice(0, m)]).to_arrow().to_pylist()
    assert got == [len(r) for r in rows] and any(len(r) != len(r.encode()) for r in rows), "character_length: wrong result"
    arms = {"character_length": lambda: [ctx.scalar_function(FN_CHARACTER_LENGTH, [b[0]]) for b in batches], "hash_text": lambda: [ctx.hash_columns([b[0]]) for b in batches]}
    ms = run_arms(ctx, arms, runs)
    total = 4 * n + value_bytes
    out = {"character_length": stats(ms["character_length"], total + 4 * n), "hash_text": stats(ms["hash_text"], total + 8 * n)}
    print(json.dumps({"step": "strings", "value_bytes": value_bytes, "batches": len(batches), "arms": out,
                      "character_length_over_hash": out["character_length"]["median_ms"] / out["hash_text"]["median_ms"]}), flush=True)


def step_dictionary(n, runs):
    import ctypes as C
    import numpy as np
    import torch
    import dfgpu
    from dfgpu import capi
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(13)
    entries = 1_000_000
    urls, off32, values = text_batch(ctx, entries, gen, torch)
    codes = torch.randint(0, entries, (n,), dtype=torch.int32, device="cuda", generator=gen)
    torch.cuda.synchronize()
    dd, d = capi.ArrayDesc(), capi.ArrayDesc()
    dd.type, dd.length, dd.null_count, dd.values, dd.offsets, dd.values_bytes = capi.UTF8, entries, 0, values.data_ptr(), off32.data_ptr(), int(off32[-1].item())
    d.type, d.key_type, d.length, d.null_count, d.values = capi.DICTIONARY, capi.INT32, n, 0, codes.data_ptr()
    d.dictionary = C.pointer(dd)
    col = ctx.wrap_device(d, keepalive=(codes, values, off32))
    m = min(n, 1 << 20)
    per_entry = np.asarray(ctx.scalar_function(FN_CHARACTER_LENGTH, [urls]).to_arrow())
    got = np.asarray(ctx.scalar_function(FN_CHARACTER_LENGTH, [col]).slice(0, m).to_arrow())
    assert np.array_equal(got, per_entry[codes[:m].cpu().numpy()]), "dictionary: wrong result"
    ms = run_arms(ctx, {"character_length_dictionary": lambda: ctx.scalar_function(FN_CHARACTER_LENGTH, [col])}, runs)
    out = {"character_length_dictionary": dict(stats(ms["character_length_dictionary"], 8 * n, 8 * n + 8 * entries + int(off32[-1].item())), entries=entries)}
    print(json.dumps({"step": "dictionary", "arms": out}), flush=True)


def step_phone(n, runs):
    import pyarrow as pa
    import torch
    import dfgpu
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(17)
    batches = []
    for lo in range(0, n, BATCH_ROWS):
        k = min(BATCH_ROWS, n - lo)
        values = torch.randint(48, 58, (15 * k,), dtype=torch.uint8, device="cuda", generator=gen)
        off32 = (torch.arange(k + 1, dtype=torch.int64, device="cuda") * 15).to(torch.int32)
        batches.append((wrap_utf8(ctx, values, off32, k, 15 * k), off32, values))
    torch.cuda.synchronize()
    one, two = ctx.from_arrow(pa.array([1], type=pa.int64())), ctx.from_arrow(pa.array([2], type=pa.int64()))
    m = min(len(batches[0][0]), 200_000)
    rows = host_rows(batches[0][1], batches[0][2], m)
    got = ctx.scalar_function(FN_SUBSTR, [batches[0][0].slice(0, m), one, two], [False, True, True]).to_arrow().to_pylist()
    assert got == [r[:2] for r in rows], "substr: wrong result"
    arms = {"substr_1_2": lambda: [ctx.scalar_function(FN_SUBSTR, [b[0], one, two], [False, True, True]) for b in batches],
            "hash_phone": lambda: [ctx.hash_columns([b[0]]) for b in batches]}
    ms = run_arms(ctx, arms, runs)
    # needed: offsets 4 + the row's first sector (the rows are adjacent, so every line of the 15 bytes a row is fetched) + result offsets 4 + 2 result bytes;
    # on top: lengths and source positions written (8) and read (8), 64-bit offsets written and read (16)
    out = {"substr_1_2": stats(ms["substr_1_2"], (4 + 15 + 4 + 2) * n, (4 + 15 + 4 + 2 + 32) * n), "hash_phone": stats(ms["hash_phone"], (4 + 15 + 8) * n)}
    print(json.dumps({"step": "phone", "batches": len(batches), "arms": out}), flush=True)


def step_crossing(n, runs):
    import pyarrow as pa
    import torch
    import dfgpu
    ctx = dfgpu.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(19)
    lit = {v: ctx.from_arrow(pa.array([v], type=pa.int64())) for v in (-1, 3, 31)}
    default = ctx.get_option("string_wave_row_bytes")
    out = {}
    for nb in CROSSING_ROW_BYTES:
        k = (256 << 20) // nb
        col, off32, values = text_batch(ctx, k, gen, torch, nb, nb)
        torch.cuda.synchronize()
        results = {}

        def arm(fn, limit):
            def go():
                ctx.set_option("string_wave_row_bytes", limit)
                if fn == "character_length":
                    return ctx.scalar_function(FN_CHARACTER_LENGTH, [col])
                return ctx.scalar_function(FN_LEFT, [col, lit[LEFT_ARMS[fn]]], [False, True])
            return go
        arms = {f"{fn}_{kern}": arm(fn, 1 if kern == "wave" else 1 << 40) for fn in ["character_length"] + list(LEFT_ARMS) for kern in ("lane", "wave")}
        for kern in ("lane", "wave"):
            results[kern] = arms[f"character_length_{kern}"]().to_arrow()
        assert results["lane"].equals(results["wave"]), f"{nb}: the two kernels disagree"
        ms = run_arms(ctx, arms, runs)
        ctx.set_option("string_wave_row_bytes", default)
        out[str(nb)] = {a: stats(v, (4 + nb) * k) for a, v in ms.items()}
        del col, off32, values
    cross = {fn: next((nb for nb in CROSSING_ROW_BYTES if out[str(nb)][fn + "_wave"]["median_ms"] <= out[str(nb)][fn + "_lane"]["median_ms"]), None)
             for fn in ["character_length"] + list(LEFT_ARMS)}
    print(json.dumps({"step": "crossing", "arms": {"crossing": out}, "first_row_bytes_where_wave_wins": cross, "string_wave_row_bytes": default}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_fn_microbench.json"))
    ap.add_argument("--step")
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs: at least 20")
    steps = {"dates": step_dates, "strings": step_strings, "dictionary": step_dictionary, "phone": step_phone, "crossing": step_crossing}
    if a.step:
        return steps[a.step](a.rows, a.runs)
    res = {"rows": a.rows, "runs": a.runs, "arms": {}}
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--rows", str(a.rows), "--runs", str(a.runs)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"step {name} failed with exit status {r.returncode}: stopping")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"step {name} done", file=sys.stderr, flush=True)
        arms = line.pop("arms")
        twice = sorted(set(arms) & set(res["arms"]))
        if twice:
            sys.exit(f"step {name} reports arms another step reported already: {twice}")
        res["arms"].update(arms)
        line.pop("step")
        res.update(line)
        with open(a.out, "w") as f:          # after every step: a later step that fails keeps what was measured
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
