"""GZIP Parquet pages for the tests, written with Python's standard zlib and a small hand-built DEFLATE writer.

repack(src, dst, compress) rewrites an UNCOMPRESSED Parquet file (as pyarrow writes it) with codec GZIP: every page payload goes through
compress(column, page, payload) -> bytes (v2 pages: the values only, the level bytes stay raw), the page headers, column chunk offsets and
sizes follow.  The member writers below reach what pyarrow never writes: stored blocks only, fixed Huffman only, Z_HUFFMAN_ONLY / Z_RLE,
memLevel 1, small windows, sync / full flushes, several and empty members per page, optional header fields, distance-32768 / length-258
matches, and malformed members for the error tests.  inflate(page) is the check: every member of a page through zlib.decompressobj(16 + 15)."""
import struct
import zlib

# ---------------------------------------------------------------- Thrift compact protocol: a generic tree, read and written back unchanged
# a struct is a list of [field id, compact type, value]; a list is (element type, [values]); bools in structs are the types 1 / 2


def _varint(b, p):
    v = s = 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, p


def _uvarint(v):
    out = bytearray()
    while True:
        if v < 0x80:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7F) | 0x80)
        v >>= 7


def _zz(v):
    return (v >> 1) ^ -(v & 1)


def _value(b, p, t):
    if t in (1, 2):
        return t == 1, p
    if t == 3:
        return b[p], p + 1
    if t in (4, 5, 6):
        v, p = _varint(b, p)
        return _zz(v), p
    if t == 7:
        return b[p:p + 8], p + 8
    if t == 8:
        n, p = _varint(b, p)
        return bytes(b[p:p + n]), p + n
    if t in (9, 10):
        h = b[p]
        p += 1
        n, et = h >> 4, h & 15
        if n == 15:
            n, p = _varint(b, p)
        out = []
        for _ in range(n):
            if et in (1, 2):
                out.append(b[p] == 1)
                p += 1
            else:
                v, p = _value(b, p, et)
                out.append(v)
        return (et, out), p
    if t == 12:
        return read_struct(b, p)
    raise ValueError(f"thrift type {t}")


def read_struct(b, p=0):
    fields, fid = [], 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return fields, p
        d, t = h >> 4, h & 15
        if d:
            fid += d
        else:
            v, p = _varint(b, p)
            fid = _zz(v)
        v, p = _value(b, p, t)
        fields.append([fid, t, v])


def _enc_value(t, v):
    if t == 3:
        return bytes([v & 0xFF])
    if t in (4, 5, 6):
        return _uvarint((v << 1) ^ (v >> 63))
    if t == 7:
        return bytes(v)
    if t == 8:
        return _uvarint(len(v)) + v
    if t in (9, 10):
        et, items = v
        head = bytes([(len(items) << 4) | et]) if len(items) < 15 else bytes([0xF0 | et]) + _uvarint(len(items))
        return head + b"".join(bytes([1 if x else 2]) if et in (1, 2) else _enc_value(et, x) for x in items)
    if t == 12:
        return write_struct(v)
    raise ValueError(t)


def write_struct(fields):
    out, last = bytearray(), 0
    for fid, t, v in sorted(fields, key=lambda f: f[0]):
        if t in (1, 2):
            t = 1 if v else 2
        d = fid - last
        out += bytes([(d << 4) | t]) if 0 < d <= 15 else bytes([t]) + _uvarint((fid << 1) ^ (fid >> 63))
        if t not in (1, 2):
            out += _enc_value(t, v)
        last = fid
    return bytes(out + b"\x00")


def _get(fields, fid, default=None):
    for f in fields:
        if f[0] == fid:
            return f[2]
    return default


def _set(fields, fid, t, v):
    for f in fields:
        if f[0] == fid:
            f[1], f[2] = t, v
            return
    fields.append([fid, t, v])


def _drop(fields, fid):
    fields[:] = [f for f in fields if f[0] != fid]


# ---------------------------------------------------------------- re-packing an uncompressed file
GZIP = 2


def pages(path):
    """[(column, page, page type, v2 level bytes, payload)] of an uncompressed file, in file order."""
    out = []
    _walk(path, lambda c, k, payload: payload, seen=out)
    return out


def repack(src, dst, compress, v2_compressed=True):
    """compress(column, page, payload) -> the page's GZIP bytes; v2_compressed=False keeps v2 pages raw (is_compressed = false) inside GZIP chunks."""
    body = _walk(src, compress, v2_compressed)
    with open(dst, "wb") as f:
        f.write(body)


def _walk(src, compress, v2_compressed=True, seen=None):
    b = open(src, "rb").read()
    assert b[:4] == b"PAR1" and b[-4:] == b"PAR1"
    mlen = struct.unpack("<I", b[-8:-4])[0]
    fmd, _ = read_struct(b, len(b) - 8 - mlen)
    body = bytearray(b"PAR1")
    page_no = {}
    for rg in _get(fmd, 4)[1]:
        rg_start, rg_comp = None, 0
        for ci, cc in enumerate(_get(rg, 1)[1]):
            meta = _get(cc, 3)
            assert _get(meta, 4) == 0, "the source must be uncompressed"
            data_off, dict_off = _get(meta, 9), _get(meta, 11)
            start = dict_off if dict_off is not None and 0 < dict_off < data_off else data_off
            end = start + _get(meta, 7)
            new_start = len(body)
            pos, new_dict, new_data = start, None, None
            while pos < end:
                hdr, p = read_struct(b, pos)
                usize, csize, typ = _get(hdr, 2), _get(hdr, 3), _get(hdr, 1)
                payload = bytes(b[p:p + csize])
                assert usize == csize
                k = page_no.get(ci, 0)
                page_no[ci] = k + 1
                lvl = 0
                v2 = _get(hdr, 8)
                if typ == 3:
                    lvl = _get(v2, 5, 0) + _get(v2, 6, 0)
                if seen is not None:
                    seen.append((ci, k, typ, lvl, payload))
                if typ == 3 and not v2_compressed:
                    new_payload = payload
                    _set(v2, 7, 2, False)
                else:
                    new_payload = payload[:lvl] + compress(ci, k, payload[lvl:]) if typ == 3 else compress(ci, k, payload)
                    if typ == 3:
                        _set(v2, 7, 1, True)
                _set(hdr, 3, 5, len(new_payload))
                _drop(hdr, 4)                                # page CRC of the old bytes
                if typ == 2 and new_dict is None:
                    new_dict = len(body)
                elif typ in (0, 3) and new_data is None:
                    new_data = len(body)
                body += write_struct(hdr) + new_payload
                pos = p + csize
            size = len(body) - new_start
            _set(meta, 4, 5, GZIP)
            _set(meta, 7, 6, size)
            _set(meta, 9, 6, new_data)
            if new_dict is not None:
                _set(meta, 11, 6, new_dict)
            _set(cc, 2, 6, new_start)
            rg_start = new_start if rg_start is None else rg_start
            rg_comp += size
        if _get(rg, 5) is not None:
            _set(rg, 5, 6, rg_start)
        if _get(rg, 7) is not None:
            _set(rg, 7, 6, rg_comp)
    md = write_struct(fmd)
    body += md + struct.pack("<I", len(md)) + b"PAR1"
    return bytes(body)


# ---------------------------------------------------------------- gzip members
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def header(extra=None, name=None, comment=None, hcrc=False, bad_hcrc=False):
    flg = (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0) | (FHCRC if hcrc or bad_hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", 1700000000) + b"\x00\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc or bad_hcrc:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ (0x5A5A if bad_hcrc else 0))
    return h


def trailer(data):
    return struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def deflate(data, level=6, wbits=15, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush_mode=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem_level, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = bytearray()
    for i in range(0, len(data), flush_every):
        out += c.compress(data[i:i + flush_every]) + c.flush(flush_mode)
    return bytes(out + c.flush())


def member(data, hdr=None, **kw):
    return (hdr if hdr is not None else header()) + deflate(data, **kw) + trailer(data)


def members(data, parts, empty=False, **kw):
    """data split into `parts` members (and an empty member first when `empty`)."""
    cuts = [len(data) * i // parts for i in range(parts + 1)]
    out = member(b"", **kw) if empty else b""
    return out + b"".join(member(data[cuts[i]:cuts[i + 1]], **kw) for i in range(parts))


# ---------------------------------------------------------------- a hand-built DEFLATE writer (fixed Huffman codes), for matches zlib never emits and malformed streams
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                    # n bits of v, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                   # a Huffman code, most significant bit first
        self.put(int(f"{c:0{n}b}"[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def fixed_lit(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_match(w, length, dist):
    i = max(k for k in range(29) if LBASE[k] <= length) if length < 258 else 28
    fixed_lit(w, 257 + i)
    w.put(length - LBASE[i], LEXT[i])
    d = max(k for k in range(30) if DBASE[k] <= dist)
    w.code(d, 5)
    w.put(dist - DBASE[d], DEXT[d])


def far_deflate(data, block=50000):
    """Greedy fixed-Huffman DEFLATE that prefers distance-32768 / length-258 matches, then runs at distance 1; blocks of `block` output bytes."""
    w = Bits()
    i, n = 0, len(data)
    while True:
        end = min(n, i + block)
        w.put(1 if end == n else 0, 1)
        w.put(1, 2)
        while i < end:
            best = 0
            if i >= 32768:
                m = 0
                while m < 258 and i + m < n and data[i + m] == data[i - 32768 + m]:
                    m += 1
                if m >= 3:
                    fixed_match(w, m, 32768)
                    i += m
                    continue
            if i >= 1:
                m = 0
                while m < 258 and i + m < n and data[i + m] == data[i - 1]:
                    m += 1
                best = m
            if best >= 3:
                fixed_match(w, best, 1)
                i += best
            else:
                fixed_lit(w, data[i])
                i += 1
        fixed_lit(w, 256)
        if end == n:
            return w.bytes()


def inflate(page):
    """Every member of a page through zlib, as MultiGzDecoder reads them; raises on any error or trailing bytes."""
    out, rest = bytearray(), page
    while True:
        d = zlib.decompressobj(16 + 15)
        out += d.decompress(rest)
        if not d.eof:
            raise zlib.error("truncated member")
        rest = d.unused_data
        if not rest:
            return bytes(out)


# ---------------------------------------------------------------- the page shapes (name -> compress(column, page, payload))
def shapes():
    def far(data):
        return header() + far_deflate(data) + trailer(data)
    return {
        "stored": lambda c, k, d: member(d, level=0),
        "fixed": lambda c, k, d: member(d, strategy=zlib.Z_FIXED),
        "huffman_only": lambda c, k, d: member(d, strategy=zlib.Z_HUFFMAN_ONLY),
        "rle": lambda c, k, d: member(d, strategy=zlib.Z_RLE),
        "mem_level_1": lambda c, k, d: member(d, level=9, mem_level=1),
        "wbits_9": lambda c, k, d: member(d, level=9, wbits=9),
        "sync_flush": lambda c, k, d: member(d, flush_every=3000, flush_mode=zlib.Z_SYNC_FLUSH),
        "full_flush": lambda c, k, d: member(d, level=1, flush_every=5000, flush_mode=zlib.Z_FULL_FLUSH),
        "multi_member": lambda c, k, d: members(d, 3, level=4),
        "empty_member": lambda c, k, d: members(d, 2, empty=True),
        "header_fields": lambda c, k, d: member(d, hdr=header(extra=b"\x01\x02AB\x00\x07", name=b"page.bin", comment=b"written by the tests", hcrc=True)),
        "far_matches": lambda c, k, d: far(d),
    }


# ---------------------------------------------------------------- malformed members (name -> payload -> bytes); every one must fail the read with Execution
def _dynamic_head(w, hlit, hdist, cl_lens, final=1):
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w.put(final, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(19 - 4, 4)
    for s in order:
        w.put(cl_lens.get(s, 0), 3)


def _bad_body(kind):
    w = Bits()
    if kind == "btype3":
        w.put(1, 1)
        w.put(3, 2)
        w.put(0, 16)
    elif kind == "cl_oversubscribed":
        _dynamic_head(w, 257, 1, {s: 1 for s in range(19)})
        w.put(0, 32)
    elif kind == "cl_incomplete":
        _dynamic_head(w, 257, 1, {0: 2, 8: 2})
        w.put(0, 32)
    elif kind == "lit_oversubscribed":
        _dynamic_head(w, 257, 1, {0: 1, 1: 1})          # symbol 0 -> code 0, symbol 1 -> code 1: every length is 1
        for _ in range(258):
            w.code(1, 1)
        w.put(0, 32)
    elif kind == "lit_incomplete":
        _dynamic_head(w, 257, 1, {0: 1, 2: 1})          # symbol 0 -> code 0, symbol 2 -> code 1
        for i in range(258):
            w.code(1 if i in (0, 256) else 0, 1)
        w.put(0, 32)
    elif kind in ("sym286", "sym287"):
        w.put(1, 1)
        w.put(1, 2)
        fixed_lit(w, 65)
        fixed_lit(w, 286 if kind == "sym286" else 287)
        fixed_lit(w, 256)
    elif kind in ("dist30", "dist31"):
        w.put(1, 1)
        w.put(1, 2)
        fixed_lit(w, 65)
        fixed_lit(w, 257)
        w.code(30 if kind == "dist30" else 31, 5)
        fixed_lit(w, 256)
    elif kind == "dist_too_far":
        w.put(1, 1)
        w.put(1, 2)
        fixed_lit(w, 65)
        fixed_match(w, 3, 2)
        fixed_lit(w, 256)
    elif kind == "stored_nlen":
        w.put(1, 1)
        w.put(0, 2)
        w.align()
        w.put(4, 16)
        w.put(0xFFFF ^ 5, 16)
        for c in b"abcd":
            w.put(c, 8)
    return w.bytes()


def malformed():
    h = header()
    bodies = {k: (lambda k: lambda d: h + _bad_body(k) + trailer(d))(k)
              for k in ("btype3", "cl_oversubscribed", "cl_incomplete", "lit_oversubscribed", "lit_incomplete", "sym286", "sym287", "dist30", "dist31",
                        "dist_too_far", "stored_nlen")}

    def crc_bad(d):
        m = bytearray(member(d))
        m[-8] ^= 1
        return bytes(m)

    def isize_bad(d):
        m = bytearray(member(d))
        m[-4] ^= 1
        return bytes(m)

    def second_member_reaches_back(d):             # a match of the second member reaching into the first member's output
        w = Bits()
        w.put(1, 1)
        w.put(1, 2)
        fixed_match(w, 3, 1)
        fixed_lit(w, 256)
        return member(d[:-3]) + h + w.bytes() + trailer(d[-3:])

    return dict(bodies, **{
        "zlib_wrapped": lambda d: zlib.compress(d),
        "raw_deflate": lambda d: deflate(d),
        "truncated_trailer": lambda d: member(d)[:-3],
        "truncated_stream": lambda d: member(d)[:len(member(d)) // 2],
        "crc_mismatch": crc_bad,
        "isize_mismatch": isize_bad,
        "fhcrc_mismatch": lambda d: member(d, hdr=header(name=b"x", bad_hcrc=True)),
        "trailing_garbage": lambda d: member(d) + b"\x00\x01\x02",
        "trailing_partial_member": lambda d: member(d) + member(b"more")[:14],
        "short_output": lambda d: member(d[:-1]),
        "long_output": lambda d: member(d + b"\x00"),
        "second_member_reaches_back": second_member_reaches_back,
    })
