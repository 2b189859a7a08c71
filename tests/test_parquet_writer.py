"""The test-side Parquet writer (tests/parquet_writer.py) against pyarrow: every shape the device tests write reads back, through the Arrow C++
reader, as the values it was given.  The device expectations in test_gpu_parquet_encodings.py therefore rest on an independent reader."""
import decimal

import pyarrow.parquet as pq
import pytest

import parquet_writer as pw

CASES = pw.edge_cases()


def expected(col, values):
    if col.decimal:
        return [None if v is None else decimal.Decimal(v).scaleb(-col.decimal[1]) for v in values]
    return values


@pytest.mark.parametrize("name", sorted(CASES))
def test_pyarrow_reads_what_the_writer_meant(tmp_path, name):
    col, values, rgs, version = CASES[name]
    path = str(tmp_path / f"{name}.parquet")
    pw.write_column(path, col, values, rgs, version=version)
    f = pq.ParquetFile(path)
    assert f.metadata.num_row_groups == len(rgs)
    encs = {e for g in range(f.metadata.num_row_groups) for e in f.metadata.row_group(g).column(0).encodings}
    want_encs = {{"plain": "PLAIN", "dict": "RLE_DICTIONARY", "delta": "DELTA_BINARY_PACKED", "delta_length": "DELTA_LENGTH_BYTE_ARRAY",
                  "delta_byte_array": "DELTA_BYTE_ARRAY", "bss": "BYTE_STREAM_SPLIT"}[p.enc] for g in rgs for p in g}
    assert want_encs <= encs
    got = f.read().column(0).to_pylist()
    assert got == expected(col, values)


def test_block_header_carries_the_parameters():
    s = pw.delta_binary_packed(list(range(1000)), 64, block=256, miniblocks=8)
    assert s[:3] == pw.uvarint(256) + bytes([8])
    # unused miniblocks of the last block: the width byte is whatever the writer chose, no body follows
    t = pw.delta_binary_packed([1, 5, 2], 64, unused_width=0xEE)
    assert t.count(b"\xee") == 3
