"""A small Parquet writer for the tests, in plain Python: one flat column, uncompressed v1 or v2 data pages, written from the published
parquet-format specification.  It exists to reach what pyarrow does not write: DELTA_BINARY_PACKED streams with any block size and miniblock
count, unused last-block miniblocks with garbage bit widths, DELTA_BYTE_ARRAY prefixes that are not the longest common prefix, and one
column chunk that mixes a dictionary page, RLE_DICTIONARY pages and DELTA pages.  tests/test_parquet_writer.py reads every shape back with
pyarrow, so the device tests compare against values an independent reader agrees with.

    write_column(path, Col("x", INT64, nullable=True), values, [[Page("delta", 1000, block=256, miniblocks=8), Page("plain", 500)]])

`values` holds Python ints / str / bytes (None = NULL); every inner list is one row group, every Page takes the next `rows` values."""
import struct
from dataclasses import dataclass, field

BOOLEAN, INT32, INT64, FLOAT, DOUBLE, BYTE_ARRAY, FLBA = 0, 1, 2, 4, 5, 6, 7
ENC = {"plain": 0, "dict": 8, "delta": 5, "delta_length": 6, "delta_byte_array": 7, "bss": 9}


# ---------------------------------------------------------------- Thrift compact protocol
def uvarint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def zigzag(v):
    return (v << 1) ^ (v >> 63) if v >= 0 else ((-v - 1) << 1) | 1


class Struct:
    """Fields as (id, type, value): type 'i32' / 'i64' / 'bin' / 'bool' / 'struct' (a Struct) / ('list', elem_type) (a list)."""
    CT = {"bool": 1, "i32": 5, "i64": 6, "bin": 8, "list": 9, "struct": 12}

    def __init__(self, *fields):
        self.fields = [f for f in fields if f[2] is not None]

    @staticmethod
    def value(t, v):
        if t in ("i32", "i64"):
            return uvarint(zigzag(v))
        if t == "bin":
            b = v.encode() if isinstance(v, str) else v
            return uvarint(len(b)) + b
        if t == "struct":
            return v.encode()
        if isinstance(t, tuple):                       # list
            et = Struct.CT[t[1]]
            head = bytes([(len(v) << 4) | et]) if len(v) < 15 else bytes([0xF0 | et]) + uvarint(len(v))
            return head + b"".join(Struct.value(t[1], x) for x in v)
        raise AssertionError(t)

    def encode(self):
        out, last = bytearray(), 0
        for fid, t, v in sorted(self.fields, key=lambda f: f[0]):
            ct = (2 if not v else 1) if t == "bool" else Struct.CT["list" if isinstance(t, tuple) else t]
            d = fid - last
            out += bytes([(d << 4) | ct]) if 0 < d <= 15 else bytes([ct]) + uvarint(zigzag(fid))
            if t != "bool":
                out += Struct.value(t, v)
            last = fid
        return bytes(out + b"\x00")


# ---------------------------------------------------------------- encodings
def bitpack(vals, width):
    acc, nbits, out = 0, 0, bytearray()
    for v in vals:
        acc |= (v & ((1 << width) - 1)) << nbits
        nbits += width
        while nbits >= 8:
            out.append(acc & 0xFF)
            acc >>= 8
            nbits -= 8
    if nbits:
        out.append(acc & 0xFF)
    return bytes(out)


def rle_hybrid(vals, width):
    """All values as bit-packed groups of 8 (a run header per group of up to 63 groups)."""
    out = bytearray()
    for s in range(0, len(vals), 504):
        chunk = list(vals[s:s + 504])
        groups = (len(chunk) + 7) // 8
        chunk += [0] * (groups * 8 - len(chunk))
        out += uvarint((groups << 1) | 1) + bitpack(chunk, width)
    return bytes(out)


def delta_binary_packed(values, bits, block=128, miniblocks=4, unused_width=0):
    """DELTA_BINARY_PACKED of signed `bits`-bit integers; deltas wrap in `bits`-bit arithmetic.  unused_width: the bit width byte written for
    miniblocks of the last block that hold no value (any value is legal there; they have no body)."""
    assert block % 128 == 0 and block % miniblocks == 0 and (block // miniblocks) % 32 == 0
    vpm, mask = block // miniblocks, (1 << bits) - 1
    signed = lambda u: u - (1 << bits) if u >> (bits - 1) else u
    vals = [v & mask for v in values]
    out = bytearray(uvarint(block) + uvarint(miniblocks) + uvarint(len(vals)) + uvarint(zigzag(signed(vals[0]) if vals else 0)))
    deltas = [signed((vals[i] - vals[i - 1]) & mask) for i in range(1, len(vals))]
    for b in range(0, len(deltas), block):
        blk = deltas[b:b + block]
        mn = min(blk)
        adj = [(d - mn) & mask for d in blk]
        used = (len(adj) + vpm - 1) // vpm
        widths = [max(a.bit_length() for a in adj[m * vpm:(m + 1) * vpm]) if m < used else unused_width for m in range(miniblocks)]
        out += uvarint(zigzag(mn)) + bytes(widths)
        for m in range(used):
            mb = adj[m * vpm:(m + 1) * vpm]
            out += bitpack(mb + [0] * (vpm - len(mb)), widths[m])
    return bytes(out)


def delta_length_byte_array(items, **kw):
    return delta_binary_packed([len(x) for x in items], 32, **kw) + b"".join(items)


def delta_byte_array(items, prefix=None, **kw):
    """prefix(i, longest) -> the prefix length written for value i (default: the longest common prefix with value i - 1)."""
    pre, suf = [], []
    for i, x in enumerate(items):
        longest = 0
        if i:
            p = items[i - 1]
            while longest < min(len(p), len(x)) and p[longest] == x[longest]:
                longest += 1
        k = prefix(i, longest) if prefix and i else longest
        assert 0 <= k <= longest
        pre.append(k)
        suf.append(x[k:])
    return delta_binary_packed(pre, 32, **kw) + delta_length_byte_array(suf, **kw)


# ---------------------------------------------------------------- file
@dataclass
class Col:
    name: str
    ptype: int
    nullable: bool = False
    type_length: int = 0
    decimal: tuple = None          # (precision, scale)
    string: bool = False


@dataclass
class Page:
    enc: str                       # plain / dict / delta / delta_length / delta_byte_array / bss
    rows: int
    opts: dict = field(default_factory=dict)

    def __init__(self, enc, rows, **opts):
        self.enc, self.rows, self.opts = enc, rows, opts


def _bytes_of(col, v):
    if col.ptype == INT32:
        return struct.pack("<i", ((v + 2**31) % 2**32) - 2**31)
    if col.ptype == INT64:
        return struct.pack("<q", ((v + 2**63) % 2**64) - 2**63)
    if col.ptype == FLOAT:
        return struct.pack("<f", v)
    if col.ptype == DOUBLE:
        return struct.pack("<d", v)
    if col.ptype == FLBA:
        return (v % (1 << (8 * col.type_length))).to_bytes(col.type_length, "big")
    return v.encode() if isinstance(v, str) else bytes(v)


def _encode_values(col, vals, page, dictionary):
    kw = {k: page.opts[k] for k in ("block", "miniblocks", "unused_width") if k in page.opts}
    if page.enc == "plain":
        if col.ptype == BYTE_ARRAY:
            return b"".join(struct.pack("<I", len(b)) + b for b in (_bytes_of(col, v) for v in vals))
        return b"".join(_bytes_of(col, v) for v in vals)
    if page.enc == "dict":
        w = max(1, (len(dictionary) - 1).bit_length())
        return bytes([w]) + rle_hybrid([dictionary[v] for v in vals], w)
    if page.enc == "delta":
        return delta_binary_packed(list(vals), 32 if col.ptype == INT32 else 64, **kw)
    if page.enc == "delta_length":
        return delta_length_byte_array([_bytes_of(col, v) for v in vals], **kw)
    if page.enc == "delta_byte_array":
        return delta_byte_array([_bytes_of(col, v) for v in vals], prefix=page.opts.get("prefix"), **kw)
    if page.enc == "bss":
        raw = [_bytes_of(col, v) for v in vals]
        w = len(raw[0]) if raw else 0
        return b"".join(bytes(r[b] for r in raw) for b in range(w))
    raise AssertionError(page.enc)


def write_column(path, col, values, row_groups, version=1, created_by="dfgpu tests/parquet_writer.py", mutate=None):
    """mutate(i, encoded values of data page i) -> the bytes written instead (malformed pages for the tests)."""
    body, rgs, at, page_no = bytearray(b"PAR1"), [], 0, 0
    for pages in row_groups:
        n_rg = sum(p.rows for p in pages)
        rg_vals = values[at:at + n_rg]
        at += n_rg
        start = len(body)
        dict_off = None
        dict_vals = sorted({v for p, s in _slices(pages) if p.enc == "dict" for v in rg_vals[s] if v is not None}, key=repr)
        dictionary = {v: i for i, v in enumerate(dict_vals)}
        if any(p.enc == "dict" for p in pages):
            payload = _encode_values(col, dict_vals, Page("plain", len(dict_vals)), None)
            hdr = Struct((1, "i32", 2), (2, "i32", len(payload)), (3, "i32", len(payload)), (7, "struct", Struct((1, "i32", len(dict_vals)), (2, "i32", 0)))).encode()
            dict_off = len(body)
            body += hdr + payload
        data_off = len(body)
        encs = set()
        for p, s in _slices(pages):
            vals = rg_vals[s]
            nonnull = [v for v in vals if v is not None]
            enc_vals = _encode_values(col, nonnull, p, dictionary)
            if mutate:
                enc_vals = mutate(page_no, enc_vals)
            page_no += 1
            encs.add(ENC[p.enc])
            defs = rle_hybrid([0 if v is None else 1 for v in vals], 1) if col.nullable else b""
            if version == 1:
                payload = (struct.pack("<I", len(defs)) + defs if col.nullable else b"") + enc_vals
                dph = Struct((1, "i32", len(vals)), (2, "i32", ENC[p.enc]), (3, "i32", 3), (4, "i32", 3))
                hdr = Struct((1, "i32", 0), (2, "i32", len(payload)), (3, "i32", len(payload)), (5, "struct", dph)).encode()
            else:
                payload = defs + enc_vals
                dph = Struct((1, "i32", len(vals)), (2, "i32", len(vals) - len(nonnull)), (3, "i32", len(vals)), (4, "i32", ENC[p.enc]),
                             (5, "i32", len(defs)), (6, "i32", 0), (7, "bool", False))
                hdr = Struct((1, "i32", 3), (2, "i32", len(payload)), (3, "i32", len(payload)), (8, "struct", dph)).encode()
            body += hdr + payload
        size = len(body) - start
        meta = Struct((1, "i32", col.ptype), (2, ("list", "i32"), sorted(encs | {3})), (3, ("list", "bin"), [col.name]), (4, "i32", 0),
                      (5, "i64", n_rg), (6, "i64", size), (7, "i64", size), (9, "i64", data_off), (11, "i64", dict_off))
        rgs.append(Struct((1, ("list", "struct"), [Struct((2, "i64", start), (3, "struct", meta))]), (2, "i64", size), (3, "i64", n_rg)))
    assert at == len(values)
    conv = 0 if col.string else (5 if col.decimal else None)
    leaf = Struct((1, "i32", col.ptype), (2, "i32", col.type_length or None), (3, "i32", 1 if col.nullable else 0), (4, "bin", col.name),
                  (6, "i32", conv), (7, "i32", col.decimal[1] if col.decimal else None), (8, "i32", col.decimal[0] if col.decimal else None))
    root = Struct((4, "bin", "schema"), (5, "i32", 1))
    fmd = Struct((1, "i32", 1), (2, ("list", "struct"), [root, leaf]), (3, "i64", len(values)), (4, ("list", "struct"), rgs), (6, "bin", created_by)).encode()
    body += fmd + struct.pack("<I", len(fmd)) + b"PAR1"
    with open(path, "wb") as f:
        f.write(bytes(body))


def _slices(pages):
    at = 0
    for p in pages:
        yield p, slice(at, at + p.rows)
        at += p.rows


# ---------------------------------------------------------------- the shapes the tests write (name -> (Col, values, row groups, page version))
def edge_cases():
    import random
    r = random.Random(3)
    I64_MIN, I64_MAX, I32_MIN, I32_MAX = -2**63, 2**63 - 1, -2**31, 2**31 - 1
    cases = {}
    ints = [r.randrange(-10**6, 10**6) for _ in range(5000)]
    nulls = [None if r.random() < 0.2 else v for v in ints]
    for block, mb in ((128, 4), (256, 8), (128, 1), (512, 4), (1024, 32)):
        cases[f"dbp_i64_{block}_{mb}"] = (Col("x", INT64), ints, [[Page("delta", 3000, block=block, miniblocks=mb), Page("delta", 2000, block=block, miniblocks=mb)]], 1)
    cases["dbp_i32_nulls_256_8_v2"] = (Col("x", INT32, nullable=True), nulls, [[Page("delta", 2600, block=256, miniblocks=8), Page("delta", 2400, block=256, miniblocks=8)]], 2)
    cases["dbp_i64_nulls_v1"] = (Col("x", INT64, nullable=True), nulls, [[Page("delta", 5000, block=512, miniblocks=4)]], 1)
    # 130 values: the last block's miniblocks 1..3 hold none, their widths are garbage and they have no body
    cases["dbp_unused_garbage_widths"] = (Col("x", INT64), ints[:130], [[Page("delta", 130, unused_width=0xFF)]], 1)
    cases["dbp_i32_unused_garbage_widths"] = (Col("x", INT32), ints[:300], [[Page("delta", 300, block=256, miniblocks=8, unused_width=200)]], 1)
    cases["dbp_width0_constant"] = (Col("x", INT64), [42] * 3000, [[Page("delta", 3000)]], 1)
    cases["dbp_arith_width0"] = (Col("x", INT32), [7 * i - 5 for i in range(3000)], [[Page("delta", 3000, block=128, miniblocks=1)]], 1)
    cases["dbp_i64_full_width_wrap"] = (Col("x", INT64), [I64_MIN if i % 2 else I64_MAX for i in range(2500)], [[Page("delta", 2500)]], 1)
    cases["dbp_i32_full_width_wrap"] = (Col("x", INT32), [I32_MIN if i % 3 else I32_MAX for i in range(2500)], [[Page("delta", 2500, block=256, miniblocks=8)]], 2)
    cases["dbp_single_value_pages"] = (Col("x", INT64, nullable=True), [5, None, -9, 11], [[Page("delta", 1), Page("delta", 1), Page("delta", 1), Page("delta", 1)]], 1)
    cases["dbp_all_null_page"] = (Col("x", INT64, nullable=True), [None] * 300 + ints[:300], [[Page("delta", 300), Page("delta", 300)]], 2)
    words = ["", "a", "ab", "abc", "abd", "b", "déjà vu", "x" * 70, "zz"]
    strs = [r.choice(words) + str(r.randrange(100)) * r.randrange(3) for _ in range(4000)]
    snull = [None if r.random() < 0.25 else s for s in strs]
    cases["dlba_256_8"] = (Col("s", BYTE_ARRAY, string=True), strs, [[Page("delta_length", 2500, block=256, miniblocks=8), Page("delta_length", 1500)]], 1)
    cases["dlba_nulls_v2"] = (Col("s", BYTE_ARRAY, nullable=True, string=True), snull, [[Page("delta_length", 4000, block=128, miniblocks=1)]], 2)
    srt = sorted(strs)
    cases["dba_sorted_512_4"] = (Col("s", BYTE_ARRAY, string=True), srt, [[Page("delta_byte_array", 4000, block=512, miniblocks=4)]], 1)
    cases["dba_short_prefixes"] = (Col("s", BYTE_ARRAY, nullable=True, string=True), [None if i % 7 == 3 else s for i, s in enumerate(srt)],
                                   [[Page("delta_byte_array", 2000, prefix=lambda i, k: k // 2), Page("delta_byte_array", 2000, prefix=lambda i, k: k if i % 3 else 0)]], 2)
    inc = ["p" * i for i in range(1, 600)]                                # every value extends the one before: the chain is as long as the value
    dec = [("q" * (600 - i)) + "r" for i in range(600)]                   # strictly decreasing prefixes
    cases["dba_increasing_prefixes"] = (Col("s", BYTE_ARRAY, string=True), inc, [[Page("delta_byte_array", 599)]], 1)
    cases["dba_decreasing_prefixes"] = (Col("s", BYTE_ARRAY, string=True), dec, [[Page("delta_byte_array", 600)]], 1)
    saw = [("m" * (i % 40)) + chr(97 + i % 26) * (i % 5) for i in range(3000)]
    cases["dba_sawtooth_prefixes"] = (Col("s", BYTE_ARRAY, string=True), saw, [[Page("delta_byte_array", 3000, block=256, miniblocks=8)]], 2)
    decs = [r.randrange(-10**20, 10**20) for _ in range(2000)]
    cases["dba_flba_decimal"] = (Col("d", FLBA, nullable=True, type_length=11, decimal=(25, 3)), [None if i % 9 == 0 else v for i, v in enumerate(sorted(decs))],
                                 [[Page("delta_byte_array", 1200), Page("delta_byte_array", 800)]], 1)
    cases["bss_flba_decimal"] = (Col("d", FLBA, nullable=True, type_length=11, decimal=(25, 3)), [None if i % 9 == 0 else v for i, v in enumerate(decs)],
                                 [[Page("bss", 1200), Page("bss", 800)]], 2)
    cases["bss_i32_nulls"] = (Col("x", INT32, nullable=True), nulls, [[Page("bss", 5000)]], 1)
    cases["bss_i64"] = (Col("x", INT64), ints, [[Page("bss", 3000), Page("bss", 2000)]], 2)
    # the dictionary-overflow fallback: a dictionary page, RLE_DICTIONARY pages, then DELTA pages -- in two row groups
    low = [r.choice(words) for _ in range(6000)]
    cases["dict_then_dlba"] = (Col("s", BYTE_ARRAY, nullable=True, string=True), [None if i % 11 == 0 else s for i, s in enumerate(low)],
                               [[Page("dict", 1000), Page("dict", 1000), Page("delta_length", 1000)], [Page("dict", 500), Page("delta_byte_array", 1500), Page("plain", 1000)]], 1)
    cases["dict_then_dbp"] = (Col("x", INT64, nullable=True), [None if i % 5 == 0 else v % 50 for i, v in enumerate(ints)],
                              [[Page("dict", 2000), Page("delta", 1500, block=256, miniblocks=8), Page("bss", 1500)]], 2)
    return cases
