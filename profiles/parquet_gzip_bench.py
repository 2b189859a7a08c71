"""GZIP Parquet reads on the device next to ZSTD and Snappy: the 12 M-row lineitem-shaped table of bench_workloads.py (parquet_scan_*: the same
columns and seed, 1 M-row row groups), written by pyarrow with dictionary on and off under GZIP levels 1 / 6 / 9, ZSTD and Snappy.  One process,
one GPU: every file is read from a device image, warm-up first, then the median of --reads reads that each end in a synchronise; each read is
checked against the source table; per-kernel ms come from the context profiler (one extra read).  Writes --out (JSON).

    python profiles/parquet_gzip_bench.py [--rows 12000000] [--reads 7] [--only gzip6] [--out profiles/parquet_gzip_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES = {f"{codec}_{d}": dict(compression=c, compression_level=lvl, use_dictionary=d == "dict")
         for codec, c, lvl in (("gzip1", "gzip", 1), ("gzip6", "gzip", 6), ("gzip9", "gzip", 9), ("zstd", "zstd", None), ("snappy", "snappy", None))
         for d in ("dict", "plain")}


def lineitem(nr):
    """bench_workloads.py's parquet_scan table (same generator calls, same seed)"""
    rng = np.random.default_rng(11)

    def dec(lo, hi):
        v = rng.integers(lo, hi, nr).astype(np.int64)
        buf = np.empty((nr, 2), dtype=np.int64); buf[:, 0] = v; buf[:, 1] = v >> 63
        return pa.Array.from_buffers(pa.decimal128(15, 2), nr, [None, pa.py_buffer(buf.tobytes())])
    pick = lambda words: pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(words), nr).astype(np.int32)), pa.array(words)).cast(pa.string())
    return pa.table({"l_orderkey": pa.array(np.sort(rng.integers(0, nr // 4 * 32, nr)).astype(np.int64)), "l_quantity": dec(100, 5001), "l_extendedprice": dec(90000, 10494951),
                     "l_discount": dec(0, 11), "l_shipdate": pa.array(rng.integers(8035, 10560, nr).astype(np.int32), type=pa.date32()),
                     "l_returnflag": pick(["A", "N", "R"]), "l_linestatus": pick(["F", "O"]), "l_shipmode": pick(["AIR", "FOB", "MAIL", "RAIL", "REG AIR", "SHIP", "TRUCK"])})


def same(cols, table):
    for i, c in enumerate(cols):
        a = c.to_arrow()
        if pa.types.is_dictionary(a.type):
            a = a.cast(a.type.value_type)
        w = table.column(i).combine_chunks()
        if len(a) != len(w) or not a.equals(w.cast(a.type)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=12_000_000)
    ap.add_argument("--reads", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated substrings of the file names to run")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import dfgpu
    from dfgpu.parquet import ParquetFile
    names = [n for n in FILES if not args.only or any(o in n for o in args.only.split(","))]
    table = lineitem(args.rows)
    decoded = args.rows * (8 + 3 * 16 + 4 + 3 * 4)          # bytes of the decoded columns (Utf8 as Int32 dictionary keys)
    tmp = tempfile.mkdtemp(prefix="dfgpu_gzip_bench_")
    paths = {n: os.path.join(tmp, n + ".parquet") for n in names}
    t0 = time.perf_counter()
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda n: pq.write_table(table, paths[n], row_group_size=1 << 20, **{k: v for k, v in FILES[n].items() if v is not None}), names))
    print(f"wrote {len(names)} files in {time.perf_counter() - t0:.1f} s", flush=True)
    ctx = dfgpu.Context(0)
    res = {}
    for n in names:
        f = ParquetFile(ctx, path=paths[n], stage_on_device=True)
        for _ in range(args.warmup):
            f.read(); ctx.synchronize()
        ok = same(f.read(), table); ctx.synchronize()
        ts = []
        for _ in range(args.reads):
            t1 = time.perf_counter(); f.read(); ctx.synchronize(); ts.append((time.perf_counter() - t1) * 1e3)
        ctx.profile_enable(True); ctx.profile_read(); f.read(); ctx.synchronize(); pr = ctx.profile_read(); ctx.profile_enable(False)
        f.close()
        ms = sorted(ts)[len(ts) // 2]
        res[n] = {"ok": ok, "file_MB": round(os.path.getsize(paths[n]) / 1e6, 1), "read_ms": round(ms, 3), "GBps": round(decoded / ms / 1e6, 2),
                  "reads_ms": [round(t, 3) for t in ts],
                  "kernels_ms": {k: round(v[1], 3) for k, v in sorted(pr.items(), key=lambda kv: -kv[1][1]) if not k.startswith("sync:") and v[1] >= 0.01}}
        print(n, json.dumps(res[n]), flush=True)
        os.unlink(paths[n])
    os.rmdir(tmp)
    out = {"workload": f"{args.rows} -row lineitem-shaped table of bench_workloads.py (parquet_scan_*), 1 M-row row groups, pyarrow {pa.__version__} writer, "
                       f"device image, utf8_dictionary on; median of {args.reads} reads after {args.warmup} warm-up reads",
           "decoded_bytes": decoded, "results": res}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not all(r["ok"] for r in res.values()):
        sys.exit("a read differs from the source table")


if __name__ == "__main__":
    main()
