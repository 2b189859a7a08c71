"""Writes the Parquet fixtures under tests/golden/parquet_encodings/ with pyarrow (python tests/golden/make_parquet_encoding_fixtures.py): the seeded
table of make_parquet_fixtures.table(1200), without dictionaries, every column whose type takes it written in the encoding family of the file:

  delta   integers and dates DELTA_BINARY_PACKED (decimals stored as integers too), strings DELTA_LENGTH_BYTE_ARRAY
  dba     integers DELTA_BINARY_PACKED, strings and FIXED_LEN_BYTE_ARRAY decimals DELTA_BYTE_ARRAY
  bss     floats, integers and FIXED_LEN_BYTE_ARRAY decimals BYTE_STREAM_SPLIT

each as v1 uncompressed, v2 Snappy and ZSTD pages.  A file holds its family's columns and the Boolean column (PLAIN), which keeps it small.  The expected columns are what pyarrow reads back."""
import os
import sys

import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_parquet_fixtures import table  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "parquet_encodings")
INTS = ["i8", "u8", "i16", "u16", "i32", "u32", "i64", "u64", "d32", "few_i64", "required_i64"]
STRS = ["low_card", "high_card"]


def encodings(family, schema):
    enc = {}
    for f in schema:
        t = f.type
        if f.name in INTS or (family == "delta" and pa.types.is_decimal(t) and t.precision <= 18):
            enc[f.name] = "BYTE_STREAM_SPLIT" if family == "bss" else "DELTA_BINARY_PACKED"
        elif f.name in STRS and family != "bss":
            enc[f.name] = "DELTA_LENGTH_BYTE_ARRAY" if family == "delta" else "DELTA_BYTE_ARRAY"
        elif pa.types.is_decimal(t) and family != "delta":
            enc[f.name] = "DELTA_BYTE_ARRAY" if family == "dba" else "BYTE_STREAM_SPLIT"
        elif pa.types.is_floating(t) and family == "bss":
            enc[f.name] = "BYTE_STREAM_SPLIT"
    return enc


PAGES = {"v1_uncompressed": dict(compression="none", data_page_version="1.0"), "v2_snappy": dict(compression="snappy", data_page_version="2.0"),
         "zstd": dict(compression="zstd", data_page_version="1.0")}

if __name__ == "__main__":
    os.makedirs(HERE, exist_ok=True)
    t = table(1200)
    for family in ("delta", "dba", "bss"):
        for name, kw in PAGES.items():
            path = os.path.join(HERE, f"{family}_{name}.parquet")
            if not os.path.exists(path):          # fixtures already committed stay byte for byte what they were
                enc = encodings(family, t.schema)
                pq.write_table(t.select([c for c in t.column_names if c in enc or c == "b"]), path, use_dictionary=False, column_encoding=enc, store_decimal_as_integer=family == "delta",
                               data_page_size=16384, row_group_size=700, **kw)
    for f in sorted(os.listdir(HERE)):
        print(f, os.path.getsize(os.path.join(HERE, f)))
