"""The GZIP page writer of tests/gzip_pages.py, checked on the CPU: every page it writes inflates through Python's zlib (member by member) to the
source page bytes, and pyarrow reads every file back to the source table (it accepts every shape, several members per page included).  The device tests
(test_gpu_parquet_gzip.py) rely on both."""
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import gzip_pages as gp


def source_table(n=20000, seed=3):
    rng = np.random.default_rng(seed)
    mask = rng.random(n) < 0.15
    return pa.table({
        "i32": pa.array(rng.integers(-1000, 1000, n).astype(np.int32), mask=mask),
        "i64": pa.array(np.repeat(rng.integers(-2**62, 2**62, n // 40 + 1), 40)[:n]),
        "f64": pa.array(rng.standard_normal(n)),
        "b": pa.array(rng.random(n) < 0.3, mask=mask),
        "s": pa.array([f"v{k}" * (k % 4) for k in rng.integers(0, 300, n)], mask=mask),
        "dec": pa.array(rng.integers(-10**12, 10**12, n)).cast(pa.decimal128(22, 2)),
    })


def write_source(path, t, **kw):
    kw.setdefault("use_dictionary", ["s"])
    pq.write_table(t, path, compression="none", row_group_size=7000, data_page_size=1 << 14, **kw)


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("name", sorted(gp.shapes()))
def test_shapes_inflate_to_the_source_pages(tmp_path, name, version):
    t = source_table()
    src, dst = str(tmp_path / "src.parquet"), str(tmp_path / f"{name}.parquet")
    write_source(src, t, data_page_version=version)
    gp.repack(src, dst, gp.shapes()[name])
    before, after = gp.pages(src), _gzip_pages(dst)
    assert len(before) == len(after) > 10
    for (c, k, typ, lvl, raw), payload in zip(before, after):
        assert payload[:lvl] == raw[:lvl]
        assert gp.inflate(payload[lvl:]) == raw[lvl:], (name, c, k)
    assert pq.ParquetFile(dst).metadata.row_group(0).column(0).compression == "GZIP"
    assert pq.read_table(dst).equals(t)             # pyarrow accepts every shape, multi-member pages included


def test_far_matches_reach_32768_back_with_length_258(tmp_path):
    rng = np.random.default_rng(1)
    block = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    data = block * 3 + b"\x07" * 5000
    body = gp.far_deflate(data)
    assert zlib.decompress(body, -15) == data
    assert len(body) < len(block) * 1.2 + 2000               # the second and third copies are matches


def test_v2_pages_can_stay_uncompressed(tmp_path):
    t = source_table(5000)
    src, dst = str(tmp_path / "src.parquet"), str(tmp_path / "v2raw.parquet")
    write_source(src, t, data_page_version="2.0")
    gp.repack(src, dst, gp.shapes()["fixed"], v2_compressed=False)
    assert pq.read_table(dst).equals(pq.read_table(src))


@pytest.mark.parametrize("name", sorted(gp.malformed()))
def test_malformed_members_fail_in_zlib(name):
    data = bytes(range(256)) * 8
    page = gp.malformed()[name](data)
    with pytest.raises(zlib.error):
        if gp.inflate(page) != data:
            raise zlib.error("different output")


def _gzip_pages(path):
    """payloads of a GZIP file, in file order (the walker of gzip_pages reads headers only; the payload is handed through unchanged)."""
    out = []
    b = open(path, "rb").read()
    import struct
    mlen = struct.unpack("<I", b[-8:-4])[0]
    fmd, _ = gp.read_struct(b, len(b) - 8 - mlen)
    for rg in gp._get(fmd, 4)[1]:
        for cc in gp._get(rg, 1)[1]:
            meta = gp._get(cc, 3)
            data_off, dict_off = gp._get(meta, 9), gp._get(meta, 11)
            pos = dict_off if dict_off is not None and 0 < dict_off < data_off else data_off
            end = pos + gp._get(meta, 7)
            while pos < end:
                hdr, p = gp.read_struct(b, pos)
                out.append(b[p:p + gp._get(hdr, 3)])
                pos = p + gp._get(hdr, 3)
    return out
