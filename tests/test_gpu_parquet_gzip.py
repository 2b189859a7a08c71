"""-m gpu: GZIP Parquet pages decoded on the device (csrc/parquet.hip k_pq_gzip, csrc/inflate_device.h) against pyarrow reading the same file,
bit-exact by the rules of test_gpu_parquet.same_column, with host and device file images and both Utf8 modes.

Files: pyarrow's own GZIP output at levels 1 / 6 / 9 (dictionary on and off, v1 and v2 pages, 64 KB and 1 MB pages, every flat type the scan
reads), the page shapes of tests/gzip_pages.py that pyarrow never writes (stored / fixed / Huffman-only / RLE blocks, memLevel 1, small windows,
flushes, several and empty members, header fields, distance-32768 matches), a seeded sweep of zlib parameters, a ~1 M-row file, a ParquetExec
plan, and malformed members: each fails the read with Execution while an intact column of the same file still reads."""
import os
import random
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq
import pytest

import gzip_pages as gp
from test_gpu_parquet import big_table, same_column

pytestmark = pytest.mark.gpu


def typed_table(n, seed=11):
    rng = np.random.default_rng(seed)
    mask = rng.random(n) < 0.12
    mask[n // 3:n // 3 + 30000] = True                        # whole pages of NULLs
    words = np.array(["", "AIR", "MAIL", "déjà vu", "日本語", "x" * 40])
    return pa.table({
        "i32": pa.array(rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), mask=mask),
        "i64": pa.array(np.sort(rng.integers(-2**40, 2**40, n))),
        "f32": pa.array(rng.random(n).astype(np.float32), mask=mask),
        "f64": pa.array(rng.standard_normal(n)),
        "b": pa.array(rng.random(n) < 0.4, mask=mask),
        "d": pa.array(rng.integers(8000, 11000, n).astype(np.int32), type=pa.date32(), mask=mask),
        "dec": pa.array(rng.integers(-10**15, 10**15, n)).cast(pa.decimal128(22, 2)),
        "s_dict": pa.array(words[rng.integers(0, len(words), n)], mask=mask),
        "s_plain": pa.array([f"{w}{v}" for w, v in zip(words[rng.integers(0, len(words), n)], rng.integers(0, 10**9, n))], mask=mask),
    })


def check_file(ctx, path, want=None, row_groups=True):
    from dfgpu.parquet import ParquetFile
    want = pq.read_table(path) if want is None else want
    for staged in (False, True):
        for as_dict in (True, False):
            f = ParquetFile(ctx, path=path, stage_on_device=staged, utf8_dictionary=as_dict)
            got = f.read()
            assert len(got) == want.num_columns
            for i, a in enumerate(got):
                name = f.column_names()[i]
                assert a.type == f.column_type(i)[0], name
                same_column(a.to_arrow(), want[name], f"{name} staged={staged} dict={as_dict}")
            if row_groups and staged:
                off = 0
                for g in range(f.num_row_groups):
                    for i, a in enumerate(f.read(g, 1)):
                        same_column(a.to_arrow(), want[f.column_names()[i]].slice(off, f.row_group_rows(g)), f"rg{g}")
                    off += f.row_group_rows(g)
            f.close()
    ctx.synchronize()


@pytest.mark.parametrize("page", [1 << 16, 1 << 20], ids=["64k-pages", "1m-pages"])
@pytest.mark.parametrize("version", ["1.0", "2.0"], ids=["v1", "v2"])
@pytest.mark.parametrize("dictionary", [True, False], ids=["dict", "plain"])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_pyarrow_gzip_files_equal_pyarrow(ctx, tmp_path, level, dictionary, version, page):
    t = typed_table(240000)
    path = str(tmp_path / "t.parquet")
    pq.write_table(t, path, compression="gzip", compression_level=level, use_dictionary=["s_dict"] + (["i32", "f64", "d"] if dictionary else []),
                   data_page_version=version, data_page_size=page, row_group_size=80000)
    assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "GZIP"
    check_file(ctx, path, t)


@pytest.fixture(scope="module")
def plain_source(tmp_path_factory):
    out = {}
    for version in ("1.0", "2.0"):
        path = str(tmp_path_factory.mktemp("src") / f"src_{version}.parquet")
        t = typed_table(150000, seed=5)
        pq.write_table(t, path, compression="none", use_dictionary=["s_dict"], data_page_version=version, data_page_size=300000, row_group_size=60000)
        out[version] = (path, t)
    return out


@pytest.mark.parametrize("version", ["1.0", "2.0"], ids=["v1", "v2"])
@pytest.mark.parametrize("name", sorted(gp.shapes()))
def test_helper_shapes_equal_pyarrow(ctx, tmp_path, plain_source, name, version):
    src, t = plain_source[version]
    path = str(tmp_path / f"{name}.parquet")
    gp.repack(src, path, gp.shapes()[name])
    check_file(ctx, path, t)


def test_v2_pages_marked_uncompressed_in_a_gzip_chunk(ctx, tmp_path, plain_source):
    src, t = plain_source["2.0"]
    path = str(tmp_path / "v2raw.parquet")
    gp.repack(src, path, gp.shapes()["fixed"], v2_compressed=False)
    check_file(ctx, path, t, row_groups=False)


def test_far_matches_and_runs_in_large_pages(ctx, tmp_path):
    """distance-32768 / length-258 matches (read back from HBM: further than the LDS ring) and distance-1 runs, over several blocks per page"""
    rng = np.random.default_rng(2)
    period = rng.integers(-2**62, 2**62, 4096)                 # 32 KB of PLAIN Int64 values, repeated
    n = 400000
    vals = np.tile(period, n // 4096 + 1)[:n]
    vals[100000:180000] = 7                                    # runs
    t = pa.table({"x": pa.array(vals), "y": pa.array(np.arange(n, dtype=np.int32))})
    src, path = str(tmp_path / "src.parquet"), str(tmp_path / "far.parquet")
    pq.write_table(t, src, compression="none", use_dictionary=False, data_page_size=1 << 20, row_group_size=n)
    gp.repack(src, path, gp.shapes()["far_matches"])
    check_file(ctx, path, t, row_groups=False)


def test_million_rows(ctx, tmp_path):
    t = big_table(1_000_000, seed=3)
    path = str(tmp_path / "big.parquet")
    pq.write_table(t, path, compression="gzip", row_group_size=250000)
    from dfgpu.parquet import ParquetFile
    f = ParquetFile(ctx, path=path, stage_on_device=True)
    assert f.num_row_groups == 4
    for name, a in zip(f.column_names(), f.read()):
        same_column(a.to_arrow(), t[name], name)
    for name, a in zip(["l_comment", "l_nullable"], f.read(1, 2, ["l_comment", "l_nullable"])):
        same_column(a.to_arrow(), t[name].slice(250000, 500000), name)


def test_parquet_exec_over_gzip_feeds_filter_and_aggregate(ctx, tmp_path):
    from dfgpu import capi, physical_plan as ops
    from dfgpu.parquet import ParquetFile
    t = big_table(400000, seed=9)
    path = str(tmp_path / "li.parquet")
    pq.write_table(t, path, row_group_size=50000, compression="gzip")
    f = ParquetFile(ctx, path=path, stage_on_device=True)
    C, F, lit = ops.Column, ops.Field, ops.Literal
    scan = ops.ParquetExec(f, ["l_orderkey", "l_quantity", "l_shipdate", "l_returnflag", "l_shipmode"], partitions=2, row_groups_per_batch=2, prune=[("l_orderkey", 0, 30000)])
    pred = ops.BinaryExpr(ops.BinaryExpr(ops.BinaryExpr(C("l_shipdate", 2), "<=", lit(9500, pa.date32())), "AND", ops.BinaryExpr(C("l_shipmode", 4), "=", lit("MAIL", pa.string()))),
                          "AND", ops.BinaryExpr(C("l_orderkey", 0), "<=", lit(30000, pa.int64())))
    agg = ops.AggregateExec("Single", [(C("l_returnflag", 3), "l_returnflag")],
                            [ops.AggregateFunctionExpr("COUNT", None, "n"), ops.AggregateFunctionExpr("SUM", ops.CastExpr(C("l_quantity", 1), capi.INT64), "q", input_field=F("l_quantity", capi.INT64))],
                            ops.CoalescePartitionsExec(ops.FilterExec(pred, scan)))
    tc = ops.TaskContext(ctx, 8192)
    out = pa.concat_tables([b.to_arrow() for b in agg.execute(0, tc)])
    sel = t.filter(pc.and_(pc.and_(pc.less_equal(t["l_shipdate"], pa.scalar(9500, pa.int32()).cast(pa.date32())), pc.equal(t["l_shipmode"], "MAIL")), pc.less_equal(t["l_orderkey"], 30000)))
    want = sel.group_by("l_returnflag").aggregate([([], "count_all"), ("l_quantity", "sum")])
    g = {r["l_returnflag"]: (r["n"], r["q"]) for r in out.to_pylist()}
    w = {r["l_returnflag"]: (r["count_all"], r["l_quantity_sum"]) for r in want.to_pylist()}
    assert g == w and len(g) == 4
    assert scan.row_groups_pruned(tc) >= 4


@pytest.fixture(scope="module")
def two_columns(tmp_path_factory):
    rng = np.random.default_rng(8)
    n = 30000
    t = pa.table({"x": pa.array(rng.integers(0, 1000, n)), "y": pa.array([f"s{v}" for v in rng.integers(0, 500, n)])})
    path = str(tmp_path_factory.mktemp("mal") / "src.parquet")
    pq.write_table(t, path, compression="none", use_dictionary=False, data_page_size=1 << 16, row_group_size=n)
    return path, t


@pytest.mark.parametrize("staged", [False, True], ids=["host-image", "device-image"])
@pytest.mark.parametrize("name", sorted(gp.malformed()))
def test_malformed_member_raises_execution_and_the_other_column_reads(ctx, tmp_path, two_columns, name, staged):
    import dfgpu
    from dfgpu.parquet import ParquetFile
    src, t = two_columns
    path = str(tmp_path / f"{name}.parquet")
    bad = gp.malformed()[name]
    gp.repack(src, path, lambda c, k, d: bad(d) if (c, k) == (0, 1) else gp.member(d))
    f = ParquetFile(ctx, path=path, stage_on_device=staged)
    with pytest.raises(dfgpu.DfgpuError) as e:
        f.read(columns=["x"])
    assert e.value.kind == "Execution", (name, e.value)
    same_column(f.read(columns=["y"])[0].to_arrow(), t["y"])
    with pytest.raises(dfgpu.DfgpuError) as e:                 # every column of the read: the intact one does not hide the bad page
        f.read(columns=["y", "x"])
    assert e.value.kind == "Execution"
    same_column(f.read(columns=["y"])[0].to_arrow(), t["y"])


STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


@pytest.mark.parametrize("seed", range(8))
def test_random_zlib_parameter_sweep(ctx, tmp_path, seed):
    r = random.Random(seed)
    n = r.choice([5000, 60000, 200000])
    t = typed_table(n, seed=seed + 100)
    keep = r.sample(t.column_names, 4)
    t = t.select(keep)
    src, path = str(tmp_path / "src.parquet"), str(tmp_path / "sweep.parquet")
    pq.write_table(t, src, compression="none", use_dictionary=[c for c in keep if r.random() < 0.5], data_page_version=r.choice(["1.0", "2.0"]),
                   data_page_size=r.choice([1 << 12, 1 << 16, 1 << 20]), row_group_size=r.choice([n, n // 3 + 1]))
    params = {}

    def comp(c, k, d):
        p = params.setdefault((c, k), dict(level=r.randrange(0, 10), wbits=r.randrange(9, 16), mem_level=r.randrange(1, 10), strategy=r.choice(STRATEGIES),
                                           flush_every=r.choice([0, 0, 700, 9000]), flush_mode=r.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])))
        parts = r.choice([1, 1, 1, 2, 3])
        return gp.members(d, parts, **p) if parts > 1 else gp.member(d, **p)
    gp.repack(src, path, comp)
    check_file(ctx, path, t, row_groups=False)


@pytest.mark.skipif(not pa.Codec.is_available("brotli"), reason="pyarrow built without Brotli")
def test_brotli_still_not_implemented(ctx, tmp_path):
    import dfgpu
    from dfgpu.parquet import ParquetFile
    path = str(tmp_path / "br.parquet")
    pq.write_table(pa.table({"x": pa.array(np.arange(1000))}), path, compression="brotli")
    f = ParquetFile(ctx, path=path, stage_on_device=True)
    with pytest.raises(dfgpu.DfgpuError) as e:
        f.read()
    assert e.value.kind == "NotImplemented" and "GZIP" in str(e.value)
