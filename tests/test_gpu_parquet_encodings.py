"""-m gpu: DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and BYTE_STREAM_SPLIT pages decoded on the device (csrc/parquet.hip:
k_pq_delta, k_pq_delta_str, k_pq_dba_chars, k_pq_bss) against pyarrow reading the same file, bit-exact by the rules of test_gpu_parquet.same_column.

Files: the fixtures of tests/golden/parquet_encodings (pyarrow, three encoding families x v1 / v2 Snappy / ZSTD pages), the shapes of
tests/parquet_writer.py that pyarrow cannot write (block sizes other than 128/4, garbage widths of unused miniblocks, widths 0 and 32 / 64,
dictionary pages followed by DELTA pages, adversarial prefix chains), and a ~1 M-row file written at test time."""
import glob
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq
import pytest

import parquet_writer as pw
from test_gpu_parquet import same_column

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parquet_encodings")
FILES = sorted(glob.glob(os.path.join(HERE, "*.parquet")))
CASES = pw.edge_cases()


def read_all(ctx, path, staged, as_dict, **kw):
    from dfgpu.parquet import ParquetFile
    f = ParquetFile(ctx, path=path, stage_on_device=staged, utf8_dictionary=as_dict, **kw)
    return f, f.read()


def test_fixtures_exist():
    assert len(FILES) == 9


@pytest.mark.parametrize("staged", [False, True], ids=["host-image", "device-image"])
@pytest.mark.parametrize("as_dict", [True, False], ids=["utf8-dictionary", "utf8-plain"])
@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-8] for f in FILES])
def test_fixture_columns_equal_pyarrow(ctx, path, as_dict, staged):
    want = pq.read_table(path)
    f, got = read_all(ctx, path, staged, as_dict)
    assert len(got) == want.num_columns
    for i, a in enumerate(got):
        name = f.column_names()[i]
        assert a.type == f.column_type(i)[0], name
        same_column(a.to_arrow(), want[name], name)
    off = 0
    for g in range(f.num_row_groups):                       # row group by row group == the matching slice
        for i, a in enumerate(f.read(g, 1)):
            same_column(a.to_arrow(), want[f.column_names()[i]].slice(off, f.row_group_rows(g)), f"rg{g}")
        off += f.row_group_rows(g)


@pytest.mark.parametrize("name", sorted(CASES))
def test_writer_shapes_equal_pyarrow(ctx, tmp_path, name):
    col, values, rgs, version = CASES[name]
    path = str(tmp_path / f"{name}.parquet")
    pw.write_column(path, col, values, rgs, version=version)
    want = pq.read_table(path)
    for staged in (False, True):
        for as_dict in ((True, False) if col.string else (True,)):
            f, got = read_all(ctx, path, staged, as_dict)
            same_column(got[0].to_arrow(), want[col.name], f"{name} staged={staged} dict={as_dict}")
            if len(rgs) > 1:
                off = 0
                for g in range(len(rgs)):
                    same_column(f.read(g, 1)[0].to_arrow(), want[col.name].slice(off, f.row_group_rows(g)), f"{name} rg{g}")
                    off += f.row_group_rows(g)
            f.close()


def big_encoded_table(n, seed=23):
    rng = np.random.default_rng(seed)
    long_rows = set(range(12345, n, 250000))
    words = np.array(["", "a", "ÄÖÜ-straße", "日本語テキスト", "MAIL", "TRUCK", "emoji 🙂"])
    s = [("L" * 70000 + str(i)) if i in long_rows else f"{words[k]}{v}" for i, (k, v) in enumerate(zip(rng.integers(0, len(words), n), rng.integers(0, 1000, n)))]
    nullmask = rng.random(n) < 0.1
    nullmask[300000:340000] = True                                   # whole pages of NULLs
    return pa.table({
        "wrap64": pa.array(np.where(np.arange(n) % 2 == 0, np.iinfo(np.int64).min, np.iinfo(np.int64).max)),
        "sorted32": pa.array(np.sort(rng.integers(-2**31, 2**31 - 1, n)).astype(np.int32)),
        "date": pa.array(rng.integers(8000, 11000, n).astype(np.int32), type=pa.date32(), mask=nullmask),
        "noisy64": pa.array(rng.integers(-2**62, 2**62, n), mask=nullmask),
        "f64": pa.array(rng.standard_normal(n), mask=nullmask),
        "f32": pa.array(rng.random(n).astype(np.float32)),
        "s_dlba": pa.array(s, mask=nullmask),
        "s_dba": pa.array(sorted(s)),
        "dec": pa.array(rng.integers(-10**15, 10**15, n)).cast(pa.decimal128(22, 2)),
    })


BIG_ENC = {"wrap64": "DELTA_BINARY_PACKED", "sorted32": "DELTA_BINARY_PACKED", "date": "DELTA_BINARY_PACKED", "noisy64": "DELTA_BINARY_PACKED",
           "f64": "BYTE_STREAM_SPLIT", "f32": "BYTE_STREAM_SPLIT", "s_dlba": "DELTA_LENGTH_BYTE_ARRAY", "s_dba": "DELTA_BYTE_ARRAY", "dec": "DELTA_BYTE_ARRAY"}


@pytest.mark.parametrize("kw", [dict(compression="none", data_page_version="1.0"), dict(compression="zstd", data_page_version="2.0", data_page_size=1 << 16)], ids=["v1", "v2-zstd-small-pages"])
def test_million_rows_many_pages_and_row_groups(ctx, tmp_path, kw):
    t = big_encoded_table(1_000_000)
    path = str(tmp_path / "big.parquet")
    pq.write_table(t, path, use_dictionary=False, column_encoding=BIG_ENC, row_group_size=250_000, **kw)
    want = pq.read_table(path)
    f, got = read_all(ctx, path, True, False)
    assert f.num_row_groups == 4
    for name, a in zip(f.column_names(), got):
        same_column(a.to_arrow(), want[name], name)
    part = f.read(1, 2, ["s_dba", "wrap64", "date"])
    for name, a in zip(["s_dba", "wrap64", "date"], part):
        same_column(a.to_arrow(), want[name].slice(250_000, 500_000), name)


def test_parquet_exec_over_delta_file_matches_plain_file(ctx, tmp_path):
    """ParquetExec -> Filter -> Aggregate over the same table written PLAIN and written with DELTA / BYTE_STREAM_SPLIT pages: the same groups."""
    from dfgpu import capi, physical_plan as ops
    from dfgpu.parquet import ParquetFile
    from test_gpu_parquet import big_table
    t = big_table(300000, seed=4)
    enc = {"l_orderkey": "DELTA_BINARY_PACKED", "l_quantity": "BYTE_STREAM_SPLIT", "l_shipdate": "DELTA_BINARY_PACKED", "l_returnflag": "DELTA_BYTE_ARRAY",
           "l_shipmode": "DELTA_LENGTH_BYTE_ARRAY", "l_extendedprice": "BYTE_STREAM_SPLIT"}
    outs = []
    for kind in ("plain", "delta"):
        path = str(tmp_path / f"{kind}.parquet")
        if kind == "plain":
            pq.write_table(t, path, row_group_size=50000, use_dictionary=False)
        else:
            pq.write_table(t, path, row_group_size=50000, use_dictionary=False, column_encoding=enc, compression="snappy")
        f = ParquetFile(ctx, path=path, stage_on_device=True)
        C, F, lit = ops.Column, ops.Field, ops.Literal
        scan = ops.ParquetExec(f, ["l_orderkey", "l_quantity", "l_shipdate", "l_returnflag", "l_shipmode"], partitions=2, row_groups_per_batch=2)
        pred = ops.BinaryExpr(ops.BinaryExpr(C("l_shipdate", 2), "<=", lit(9500, pa.date32())), "AND", ops.BinaryExpr(C("l_shipmode", 4), "=", lit("MAIL", pa.string())))
        agg = ops.AggregateExec("Single", [(C("l_returnflag", 3), "l_returnflag")],
                                [ops.AggregateFunctionExpr("COUNT", None, "n"), ops.AggregateFunctionExpr("SUM", ops.CastExpr(C("l_quantity", 1), capi.INT64), "q", input_field=F("l_quantity", capi.INT64))],
                                ops.CoalescePartitionsExec(ops.FilterExec(pred, scan)))
        out = pa.concat_tables([b.to_arrow() for b in agg.execute(0, ops.TaskContext(ctx, 8192))])
        outs.append({r["l_returnflag"]: (r["n"], r["q"]) for r in out.to_pylist()})
    sel = t.filter(pc.and_(pc.less_equal(t["l_shipdate"], pa.scalar(9500, pa.int32()).cast(pa.date32())), pc.equal(t["l_shipmode"], "MAIL")))
    want = {r["l_returnflag"]: (r["count_all"], r["l_quantity_sum"]) for r in sel.group_by("l_returnflag").aggregate([([], "count_all"), ("l_quantity", "sum")]).to_pylist()}
    assert outs[0] == outs[1] == want and len(want) == 4


def _dbp_header(block, mb, total, first=0):
    return pw.uvarint(block) + pw.uvarint(mb) + pw.uvarint(total) + pw.uvarint(pw.zigzag(first))


MALFORMED = {
    # (column, values, page, mutate(encoded values) -> bytes)
    "truncated_header": (pw.Col("x", pw.INT64), list(range(300)), "delta", lambda b: b[:3]),
    "truncated_block": (pw.Col("x", pw.INT64), [i * i * 977 for i in range(300)], "delta", lambda b: b[:len(b) // 2]),
    "width_33_int32": (pw.Col("x", pw.INT32), list(range(129)), "delta", lambda b: _dbp_header(128, 4, 129) + b"\x00" + bytes([33, 0, 0, 0]) + b"\x01" * 200),
    "width_65_int64": (pw.Col("x", pw.INT64), list(range(129)), "delta", lambda b: _dbp_header(128, 4, 129) + b"\x00" + bytes([65, 0, 0, 0]) + b"\x01" * 600),
    "block_not_128_multiple": (pw.Col("x", pw.INT64), list(range(129)), "delta", lambda b: _dbp_header(100, 4, 129) + b[6:]),
    "miniblock_not_32_multiple": (pw.Col("x", pw.INT64), list(range(129)), "delta", lambda b: _dbp_header(128, 8, 129) + b[6:]),
    "count_below_non_null": (pw.Col("x", pw.INT64), list(range(300)), "delta", lambda b: pw.delta_binary_packed(list(range(150)), 64)),
    "prefix_longer_than_previous": (pw.Col("s", pw.BYTE_ARRAY, string=True), ["ab", "abc"], "delta_byte_array",
                                    lambda b: pw.delta_binary_packed([0, 5], 32) + pw.delta_length_byte_array([b"ab", b"c"])),
    "lengths_beyond_page": (pw.Col("s", pw.BYTE_ARRAY, string=True), ["abcde"] * 40, "delta_length", lambda b: b[:-20]),
    "suffixes_beyond_page": (pw.Col("s", pw.BYTE_ARRAY, string=True), [f"k{i:05d}" for i in range(300)], "delta_byte_array", lambda b: b[:-30]),
    "bss_size_not_count_times_width": (pw.Col("x", pw.INT64), list(range(300)), "bss", lambda b: b + b"\x00" * 7),
    "bss_short": (pw.Col("x", pw.INT32, nullable=True), [None if i % 3 == 0 else i for i in range(300)], "bss", lambda b: b[:-8]),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_pages_raise_execution(ctx, tmp_path, name):
    """As test_gpu_parquet.test_malformed_pages_raise_instead_of_faulting: every read is bounded by the page, the page is flagged, the read raises Execution."""
    import dfgpu
    from dfgpu.parquet import ParquetFile
    col, values, enc, mutate = MALFORMED[name]
    path = str(tmp_path / f"{name}.parquet")
    pw.write_column(path, col, values, [[pw.Page(enc, len(values))]], mutate=lambda i, b: mutate(b))
    for staged in (False, True):
        f = ParquetFile(ctx, path=path, stage_on_device=staged, utf8_dictionary=False)
        with pytest.raises(dfgpu.DfgpuError) as e:
            f.read()
            ctx.synchronize()
        assert e.value.kind == "Execution", str(e.value)
        f.close()
    # the same context still reads a good file afterwards
    good = str(tmp_path / "good.parquet")
    pw.write_column(good, col, values, [[pw.Page(enc, len(values))]])
    f = ParquetFile(ctx, path=good, stage_on_device=True, utf8_dictionary=False)
    same_column(f.read()[0].to_arrow(), pq.read_table(good)[col.name])
