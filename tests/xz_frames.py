"""Frame programs: one .xz stream (ZIP method 95, "The .xz File Format" 1.0.4) written field by field, so that every framing
field can be stated apart from the truth -- what liblzma's encoder never writes.  The LZMA2 payload of a block is liblzma's
raw encoder's or a chunk program of tests/lzma_packets.py; everything around it is written here.

    Stream(blocks, check=1, ...).write()   -> the stream's bytes
    Block(data, csize=True, usize=7, ...)  one block: flags, size fields, filter list, header padding, payload, block padding,
                                           check field -- each true by default, each overridable
    judge(x)                               liblzma's verdict (Python's lzma): (0, consumed, bytes) | (-3, ..) | (-5, len(x), ..)
    programs()                             the named families: (name, stream, what the family says: "ok" | "bad" | "short", data)
    verdicts()                             the same, judged: (name, stream, status, data, in_used)
    partials()                             {name: bytes liblzma had handed out} of the programs it wants more input for
    resealed(seed, n)                      one or two mutated framing bytes of a two-block base, the four kinds of CRC-32
                                           recomputed so that the parser gets past them: (name, stream, zones)

Every named program has ONE defect, so what liblzma must say of it is known in advance; the tests hold judge() to that and
then every decoder of this project to judge().  Test infrastructure only."""
import hashlib
import lzma
import random
import zlib

from tests import lzma_packets as K

MAGIC, FOOT_MAGIC = b"\xfd7zXZ\x00", b"YZ"
CHECK_SIZE = (0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64)
VERIFIED = (0, 1, 4, 10)
OK, DATA_ERROR, BUF_ERROR, OUT_FULL = 0, -3, -5, -200
LZMA2, DELTA, X86, POWERPC, ARM = 0x21, 0x03, 0x04, 0x05, 0x07
V63 = (1 << 63) - 1


def crc32le(b):
    return zlib.crc32(bytes(b)).to_bytes(4, "little")


def vli(v, width=0):
    """the variable-length integer of 1.2; width: that many bytes (more than v needs: not minimal, the last byte is 0)"""
    o = bytearray()
    while v >= 0x80:
        o.append((v & 0x7F) | 0x80)
        v >>= 7
    o.append(v)
    while len(o) < width:
        o[-1] |= 0x80
        o.append(0)
    return bytes(o)


def read_vli(b, p, lim):
    """-> (value, next position) or None (runs off lim, ten bytes, a zero byte that is not the first)"""
    v = 0
    for i in range(9):
        if p >= lim:
            return None
        c = b[p]
        p += 1
        if c == 0 and i:
            return None
        v |= (c & 0x7F) << (7 * i)
        if not c & 0x80:
            return v, p
    return None


def check_field(check, data):
    if check == 1:
        return crc32le(data)
    if check == 4:
        import oracle

        return oracle.crc64(data).to_bytes(8, "little")
    if check == 10:
        return hashlib.sha256(data).digest()
    return bytes((0xA5 + 7 * i) & 0xFF for i in range(CHECK_SIZE[check]))  # not verified by anyone: any bytes of the right length


def text(n, seed=1):
    """n bytes that compress: words of a small vocabulary"""
    rnd = random.Random(seed)
    words = [bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(2, 9))) for _ in range(40)]
    o = bytearray()
    while len(o) < n:
        o += rnd.choice(words) + (b" " if rnd.randrange(9) else b".\n")
    return bytes(o[:n])


def noise(n, seed=1):
    rnd = random.Random(seed)
    return bytes(rnd.randrange(256) for _ in range(n))


def raw_lzma2(data, filters=None, dict_size=1 << 16):
    """liblzma's raw encoder: the chain's output for `data` (Delta / BCJ in front of LZMA2 as given)"""
    f = [dict(id=i, **kw) for i, kw in (filters or [])] + [dict(id=lzma.FILTER_LZMA2, preset=6, dict_size=dict_size)]
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=f)


class Block:
    """One block.  Everything but `data` has a true default:
    payload     raw LZMA2 bytes that decode (through `unfilter`-ed chains: see raw_lzma2) to data; None = liblzma's encoder
    flags_or    bits OR-ed into the block flags byte (the reserved bits 0x04 .. 0x20)
    csize/usize None absent, True the true value, an int that value, bytes the field as written
    filters     [(id, property bytes)] or [(id, property bytes, property size as written)]; None = LZMA2 with dict_byte
    hpad        header padding bytes (None: up to the next multiple of four), hpad_byte their value
    hcrc_xor    XOR-ed into the header's CRC-32
    bpad_byte   value of the block padding bytes
    check       None the true field (arbitrary bytes for ids nobody verifies), bytes as written, an int XOR-ed into byte 0"""

    def __init__(self, data, payload=None, flags_or=0, csize=None, usize=None, filters=None, dict_byte=None, hpad=None, hpad_byte=0,
                 hcrc_xor=0, bpad_byte=0, check=None, enc_filters=None):
        self.data, self.flags_or, self.csize, self.usize, self.hpad, self.hpad_byte = bytes(data), flags_or, csize, usize, hpad, hpad_byte
        self.hcrc_xor, self.bpad_byte, self.check = hcrc_xor, bpad_byte, check
        self.payload = raw_lzma2(self.data, enc_filters) if payload is None else bytes(payload)
        if filters is None:
            filters = [(LZMA2, bytes([K.lzma2_dict_byte(1 << 16) if dict_byte is None else dict_byte]))]
        self.filters = filters

    def _size(self, f, true):
        if f is None:
            return b""
        if isinstance(f, (bytes, bytearray)):
            return bytes(f)
        return vli(true if f is True else f)

    def header(self):
        flags = (len(self.filters) - 1) | (0x40 if self.csize is not None else 0) | (0x80 if self.usize is not None else 0) | self.flags_or
        body = bytes([flags]) + self._size(self.csize, len(self.payload)) + self._size(self.usize, len(self.data))
        for f in self.filters:
            body += vli(f[0]) + vli(f[2] if len(f) > 2 else len(f[1])) + bytes(f[1])
        pad = -(len(body) + 1) % 4 if self.hpad is None else self.hpad
        body += bytes([self.hpad_byte]) * pad
        assert (len(body) + 1) % 4 == 0 and len(body) + 5 <= 1024, len(body)
        h = bytes([(len(body) + 5) // 4 - 1]) + body
        return h + (zlib.crc32(h) ^ self.hcrc_xor).to_bytes(4, "little")

    def write(self, check_id):
        """-> (the block's bytes, its true index record)"""
        h = self.header()
        c = self.check
        if not isinstance(c, (bytes, bytearray)):
            t = check_field(check_id, self.data)
            c = t if not c else bytes([t[0] ^ c]) + t[1:]
        return (h + self.payload + bytes([self.bpad_byte]) * (-len(self.payload) % 4) + bytes(c),
                (len(h) + len(self.payload) + len(c), len(self.data)))


class Stream:
    """head_flags / foot_flags: the two flag bytes as written (None: {0, check}); *_crc_xor: XOR-ed into that CRC-32; count /
    records: the index's record count and (unpadded size, uncompressed size) records as written (None: true); ipad_byte: the
    index padding's value; extra_index: bytes behind the records, in front of the padding; backward: the footer's backward
    size field (None: true)"""

    def __init__(self, blocks, check=1, head_flags=None, head_crc_xor=0, indicator=0, count=None, records=None, extra_index=b"", ipad_byte=0,
                 index_crc_xor=0, backward=None, foot_flags=None, foot_magic=FOOT_MAGIC, foot_crc_xor=0, trailing=b""):
        self.blocks, self.check = list(blocks), check
        self.head_flags, self.head_crc_xor, self.indicator, self.count, self.records = head_flags, head_crc_xor, indicator, count, records
        self.extra_index, self.ipad_byte, self.index_crc_xor, self.backward = extra_index, ipad_byte, index_crc_xor, backward
        self.foot_flags, self.foot_magic, self.foot_crc_xor, self.trailing = foot_flags, foot_magic, foot_crc_xor, trailing

    def data(self):
        return b"".join(b.data for b in self.blocks)

    def true_records(self):
        return [b.write(self.check)[1] for b in self.blocks]

    def layout(self):
        """-> (bytes, dict of zone -> [(start, end)]): where the framing lies (CRC fields left out)"""
        flags = bytes([0, self.check]) if self.head_flags is None else bytes(self.head_flags)
        x = bytearray(MAGIC + flags + (zlib.crc32(flags) ^ self.head_crc_xor).to_bytes(4, "little"))
        z = {"flags": [(6, 8)], "header": [], "index": [], "footer": []}
        recs = []
        for b in self.blocks:
            blk, rec = b.write(self.check)
            z["header"].append((len(x), len(x) + len(b.header()) - 4))
            x += blk
            recs.append(rec)
        recs = recs if self.records is None else self.records
        idx = bytes([self.indicator]) + vli(len(self.blocks) if self.count is None else self.count)
        idx += b"".join(vli(u) + vli(s) for u, s in recs) + bytes(self.extra_index)
        idx += bytes([self.ipad_byte]) * (-len(idx) % 4)
        z["index"].append((len(x), len(x) + len(idx)))
        x += idx + (zlib.crc32(idx) ^ self.index_crc_xor).to_bytes(4, "little")
        tail = ((len(idx) + 4) // 4 - 1 if self.backward is None else self.backward).to_bytes(4, "little")
        tail += bytes([0, self.check]) if self.foot_flags is None else bytes(self.foot_flags)
        z["footer"].append((len(x) + 4, len(x) + 12))
        x += (zlib.crc32(tail) ^ self.foot_crc_xor).to_bytes(4, "little") + tail + bytes(self.foot_magic)
        return bytes(x) + bytes(self.trailing), z

    def write(self):
        return self.layout()[0]


def split(x):
    """the reader: a valid single-stream image -> Stream whose write() gives x back (blocks keep their header fields as written)"""
    assert x[:6] == MAGIC and x[-2:] == FOOT_MAGIC
    check = x[7]
    isize = (int.from_bytes(x[-8:-4], "little") + 1) * 4
    ipos = len(x) - 12 - isize
    n, p = read_vli(x, ipos + 1, len(x))
    recs = []
    for _ in range(n):
        u, p = read_vli(x, p, len(x))
        s, p = read_vli(x, p, len(x))
        recs.append((u, s))
    pos, blocks = 12, []
    data = lzma.decompress(x, format=lzma.FORMAT_XZ)
    dpos = 0
    for u, s in recs:
        hsize = (x[pos] + 1) * 4
        flags, q, hend = x[pos + 1], pos + 2, pos + hsize - 4
        cs = us = None
        if flags & 0x40:
            q0 = q
            q = read_vli(x, q, hend)[1]
            cs = x[q0:q]
        if flags & 0x80:
            q0 = q
            q = read_vli(x, q, hend)[1]
            us = x[q0:q]
        filters = []
        for _ in range((flags & 3) + 1):
            fid, q = read_vli(x, q, hend)
            ps, q = read_vli(x, q, hend)
            filters.append((fid, x[q:q + ps]))
            q += ps
        csize = u - hsize - CHECK_SIZE[check]
        pay = x[pos + hsize:pos + hsize + csize]
        end = pos + ((u + 3) & ~3)
        blocks.append(Block(data[dpos:dpos + s], payload=pay, flags_or=flags & 0x3C, csize=cs, usize=us, filters=filters, hpad=hend - q,
                            check=x[end - CHECK_SIZE[check]:end]))
        dpos += s
        pos = end
    assert pos == ipos and dpos == len(data)
    return Stream(blocks, check=check)


def judge(x):
    """liblzma on one stream (lzma_stream_decoder without LZMA_CONCATENATED, as mz_strm_lzma.c opens it):
    (0, consumed, bytes) at the footer, (-3, None, None) refused, (-5, len(x), bytes so far) when it wants more input"""
    d = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
    try:
        out = d.decompress(bytes(x))
    except lzma.LZMAError:
        return DATA_ERROR, None, None
    if d.eof:
        return OK, len(x) - len(d.unused_data), out
    return BUF_ERROR, len(x), out


# ---- the named families ---------------------------------------------------------------------------------------------------
_cache = {}
T = text(3000, seed=7)
A, B, C3 = T[:700], T[700:1500], T[1500:1900]


def _raw_last():
    """(payload, data) of a chunk program whose last chunk is an uncompressed one"""
    rnd = random.Random(3)
    tail = bytes(rnd.randrange(256) for _ in range(37))
    p = K.ChunkProgram("frames/raw-last", [("lzma", 0xE0, K._seed_bytes(rnd, 40) + [("match", 5, 9), ("lit", 0x33)], (3, 0, 2)), ("raw", 2, tail)])
    data, v = p.expand()
    assert v is None
    return p.raw(), bytes(data)


def _with_pad(want, seed):
    """a block whose payload leaves `want` bytes of block padding"""
    for n in range(300, 420):
        b = Block(text(n, seed))
        if -len(b.payload) % 4 == want:
            return b
    raise AssertionError(want)


def _index_pad(want):
    """blocks whose true index leaves `want` padding bytes"""
    import itertools

    for n in (1, 2, 3):
        # (record fields of one and of two bytes: 20 bytes of text, 200 of them, 120 bytes of noise -- two bytes unpadded, one byte long)
        for datas in itertools.product((text(20, 20), text(200, 21), noise(120, 22)), repeat=n):
            s = Stream([Block(d) for d in datas])
            recs = s.true_records()
            if -(2 + sum(len(vli(u)) + len(vli(v)) for u, v in recs)) % 4 == want:
                return s.blocks
    raise AssertionError(want)


def programs():
    """-> [(name, stream bytes, "ok" | "bad" | "short", the data the stream was written around (None: not known))]"""
    if "programs" in _cache:
        return _cache["programs"]
    P = []

    def add(name, s, verdict):
        P.append((name, s.write() if isinstance(s, Stream) else bytes(s), verdict, s.data() if isinstance(s, Stream) else None))

    one = lambda **kw: Stream([Block(A, **kw)])
    tc, tu = len(Block(A).payload), len(A)
    # ---- sizes
    add("sizes/both", one(csize=True, usize=True), "ok")
    add("sizes/csize", one(csize=True), "ok")
    add("sizes/usize", one(usize=True), "ok")
    for d in (1, -1):
        add("sizes/csize%+d" % d, one(csize=tc + d), "bad")
        add("sizes/usize%+d" % d, one(usize=tu + d), "bad")
        add("sizes/both/csize%+d" % d, one(csize=tc + d, usize=True), "bad")
        add("sizes/both/usize%+d" % d, one(csize=True, usize=tu + d), "bad")
    add("sizes/csize-0", one(csize=0), "bad")
    add("sizes/csize-2^63-1", one(csize=V63), "bad")
    add("sizes/csize-2^63-4", one(csize=V63 - 3), "bad")
    add("sizes/usize-0-empty-block", Stream([Block(b"", usize=0)]), "ok")
    add("sizes/usize-0", one(usize=0), "bad")
    add("sizes/usize-2^63-1", one(usize=V63), "bad")
    add("sizes/csize-not-minimal", one(csize=vli(tc, 3)), "bad")
    add("sizes/usize-not-minimal", one(usize=vli(tu, 9)), "bad")
    add("sizes/usize-ten-bytes", one(usize=b"\xff" * 9 + b"\x01"), "bad")
    rp, rd = _raw_last()
    add("sizes/raw-chunk-last/both", Stream([Block(rd, payload=rp, csize=True, usize=True)]), "ok")
    add("sizes/raw-chunk-last/csize+1", Stream([Block(rd, payload=rp, csize=len(rp) + 1, usize=True)]), "bad")
    add("sizes/raw-chunk-last/usize-1", Stream([Block(rd, payload=rp, csize=True, usize=len(rd) - 1)]), "bad")
    add("sizes/second-block/both", Stream([Block(A), Block(B, csize=True, usize=True)]), "ok")
    add("sizes/second-block/usize-1", Stream([Block(A), Block(B, csize=True, usize=len(B) - 1)]), "bad")
    add("sizes/second-block/csize+1", Stream([Block(A), Block(B, csize=len(Block(B).payload) + 1)]), "bad")
    # ... that run out in the block's first chunk header, in the coder's first bytes, inside packets; in a later chunk's header
    for k in (1, 5, 11, 12, 40, len(Block(B).payload) - 2):
        add("sizes/second-block/csize-%d" % k, Stream([Block(A), Block(B, csize=k)]), "bad")
    for k in (1, 7, 300):
        add("sizes/second-block/usize-%d" % k, Stream([Block(A), Block(B, usize=k)]), "bad")
        add("sizes/usize-%d" % k, one(usize=k), "bad")
    rnd = random.Random(8)
    two_chunks = K.ChunkProgram("frames/two-chunks", [("lzma", 0xE0, K._seed_bytes(rnd, 70), (3, 0, 2)), ("lzma", 0x80, K._seed_bytes(rnd, 50)),
                                                      ("raw", 2, noise(30, 8)), ("lzma", 0xA0, K._seed_bytes(rnd, 20))])
    d2, v = two_chunks.expand()
    assert v is None
    r2 = two_chunks.raw()
    q2 = 6 + (r2[3] << 8) + r2[4] + 1                  # where the second chunk's header starts
    q3 = q2 + 5 + (r2[q2 + 3] << 8) + r2[q2 + 4] + 1   # ... and the uncompressed chunk's
    for k in (q2 - 1, q2, q2 + 1, q2 + 5, q2 + 9, q2 + 10, q2 + 14, q3 - 1, q3, q3 + 2, q3 + 3, q3 + 20, q3 + 33, q3 + 38, q3 + 39, len(r2) - 1):
        add("sizes/chunks/csize-%d" % k, Stream([Block(A[:40]), Block(bytes(d2), payload=r2, csize=k)], check=4), "bad")
    # ... that end behind an input which breaks off inside the first chunk, with a data error in front: the chunk's size field
    # (65536) and the declared 65540 both point behind the 30-odd bytes there are, and behind the 64 KiB a stream's input buffer starts with (a coder's first byte must be 0)
    head = Stream([]).write()[:12]
    cut_chunk = b"\xe0\x00\xff\xff\xff\x5d\x01"
    add("sizes/csize-behind-cut-chunk", head + Block(A, csize=65540).header() + cut_chunk, "bad")
    add("sizes/csize-behind-cut-chunk/filtered",
        head + Block(A, csize=65540, filters=[(X86, b""), (LZMA2, b"\x10")]).header() + cut_chunk, "bad")
    x1, z1 = Stream([Block(A)]).layout()
    add("sizes/csize-behind-cut-chunk/second-block", x1[:z1["index"][0][0]] + Block(B, csize=65540).header() + cut_chunk + b"\x01" * 9, "bad")
    add("sizes/chunks/both", Stream([Block(A[:40]), Block(bytes(d2), payload=r2, csize=True, usize=True)], check=4), "ok")
    # ---- header
    for bit in (0x04, 0x08, 0x10, 0x20):
        add("header/reserved-%02x" % bit, one(flags_or=bit), "bad")
    add("header/padding-4-more", one(hpad=3 + 4), "ok")
    add("header/padding-to-1024", one(hpad=1024 - 4 - 5), "ok")
    add("header/padding-to-1024/sizes", one(csize=True, usize=True, hpad=1024 - 4 - 5 - len(vli(tc)) - len(vli(tu))), "ok")
    add("header/padding-nonzero", one(hpad_byte=1), "bad")
    add("header/padding-nonzero/7", one(hpad=7, hpad_byte=0x80), "bad")
    add("header/lzma2-props-0", Stream([Block(A, filters=[(LZMA2, b"")])]), "bad")
    add("header/lzma2-props-2", Stream([Block(A, filters=[(LZMA2, bytes([K.lzma2_dict_byte(1 << 16), 0]))])]), "bad")
    for db, v in ((0, "ok"), (1, "ok"), (39, "ok"), (40, "ok"), (41, "bad"), (0x54, "bad")):
        d = A[:300]     # (a 4 KiB dictionary holds it whole)
        add("header/dict-byte-%d" % db, Stream([Block(d, payload=raw_lzma2(d, dict_size=4096), dict_byte=db)]), v)
    x86 = [(lzma.FILTER_X86, {})]
    add("header/bcj-props-1", Stream([Block(A, enc_filters=x86, filters=[(X86, b"\0"), (LZMA2, b"\x10")])]), "bad")
    four = [(lzma.FILTER_DELTA, dict(dist=3)), (lzma.FILTER_X86, {}), (lzma.FILTER_POWERPC, {})]
    fourh = [(DELTA, b"\x02"), (X86, b""), (POWERPC, b""), (LZMA2, b"\x10")]
    add("header/four-filters", Stream([Block(A, enc_filters=four, filters=fourh)]), "ok")
    add("header/filtered-then-plain", Stream([Block(A, enc_filters=x86, filters=[(X86, b""), (LZMA2, b"\x10")]), Block(B)]), "ok")
    add("header/plain-then-filtered", Stream([Block(B), Block(A, enc_filters=four, filters=fourh, usize=True)]), "ok")
    add("header/lzma2-not-last", Stream([Block(A, filters=[(LZMA2, b"\x10"), (X86, b"")])]), "bad")
    add("header/filter-id-unknown", Stream([Block(A, filters=[(0x02, b""), (LZMA2, b"\x10")])]), "bad")
    add("header/crc", one(hcrc_xor=1), "bad")
    add("header/crc/second-block", Stream([Block(A), Block(B, hcrc_xor=0x80000000)]), "bad")
    # ---- checks
    for cid in range(16):
        add("checks/id-%d" % cid, Stream([Block(A), Block(B)], check=cid), "ok")
    for cid in (1, 4, 10):
        add("checks/id-%d/wrong" % cid, Stream([Block(A, check=0x01)], check=cid), "bad")
        add("checks/id-%d/wrong-last-byte" % cid,
            Stream([Block(A, check=check_field(cid, A)[:-1] + bytes([check_field(cid, A)[-1] ^ 0x80]))], check=cid), "bad")
        add("checks/id-%d/wrong-second-block" % cid, Stream([Block(A), Block(B, check=0x10)], check=cid), "bad")
    for cid in VERIFIED:
        add("checks/id-%d/empty-block-between" % cid, Stream([Block(A), Block(b""), Block(B)], check=cid), "ok")
    # ---- padding
    for n in (1, 2, 3):
        b = _with_pad(n, 10 + n)
        add("padding/block-%d/zero" % n, Stream([b, Block(C3)]), "ok")
        add("padding/block-%d/nonzero" % n, Stream([Block(b.data, bpad_byte=1), Block(C3)]), "bad")
        add("padding/block-%d/nonzero-last-block" % n, Stream([Block(C3), Block(b.data, bpad_byte=0x80)]), "bad")
        blocks = _index_pad(n)
        add("padding/index-%d/zero" % n, Stream(blocks), "ok")
        add("padding/index-%d/nonzero" % n, Stream(blocks, ipad_byte=1), "bad")
    # ---- index
    two = [Block(A), Block(B)]
    (u1, s1), (u2, s2) = Stream(two).true_records()
    add("index/count+1", Stream(two, count=3), "bad")
    add("index/count-1", Stream(two, count=1), "bad")
    add("index/count-0", Stream(two, count=0), "bad")
    add("index/no-blocks", Stream([]), "ok")
    add("index/no-blocks/count-1", Stream([], count=1), "bad")
    add("index/extra-record", Stream(two, extra_index=vli(u2) + vli(s2)), "bad")
    add("index/records-swapped", Stream(two, records=[(u2, s2), (u1, s1)]), "bad")
    add("index/sums-still-match", Stream(two, records=[(u1 + 4, s1 - 1), (u2 - 4, s2 + 1)]), "bad")
    add("index/usize-sums-still-match", Stream(two, records=[(u1, s1 + 1), (u2, s2 - 1)]), "bad")
    b3 = _with_pad(3, 13)
    u3, s3 = Stream([b3]).true_records()[0]
    add("index/unpadded-rounded-up", Stream([b3], records=[((u3 + 3) & ~3, s3)]), "bad")
    add("index/usize-wrong", Stream(two, records=[(u1, s1), (u2, s2 + 1)]), "bad")
    add("index/crc", Stream(two, index_crc_xor=1), "bad")
    # ---- footer
    ilo, ihi = Stream(two).layout()[1]["index"][0]
    bw = (ihi - ilo + 4) // 4 - 1
    add("footer/backward+1", Stream(two, backward=bw + 1), "bad")
    add("footer/backward-1", Stream(two, backward=bw - 1), "bad")
    add("footer/flags-differ", Stream(two, check=1, foot_flags=b"\x00\x04"), "bad")
    add("footer/flags-differ-same-size", Stream(two, check=1, foot_flags=b"\x00\x02"), "bad")
    add("footer/flag-byte-0", Stream(two, foot_flags=b"\x01\x01"), "bad")
    add("footer/magic", Stream(two, foot_magic=b"YX"), "bad")
    add("footer/crc", Stream(two, foot_crc_xor=0x100), "bad")
    # ---- stream header
    add("stream-header/flag-byte-0", Stream(two, head_flags=b"\x01\x01", foot_flags=b"\x01\x01"), "bad")
    add("stream-header/check-id-high-bits", Stream(two, head_flags=b"\x00\x11", foot_flags=b"\x00\x11"), "bad")
    add("stream-header/crc", Stream(two, head_crc_xor=1), "bad")
    add("stream-header/magic", b"\xfd7zXY\x00" + Stream(two).write()[6:], "bad")
    # ---- a default-written frame around chunk programs (raw chunks, a props change, a dictionary reset in mid-block)
    rnd = random.Random(5)
    lz = lambda ctl, props=None: ("lzma", ctl, K._seed_bytes(rnd, 12) + [("match", 3, 4), ("shortrep",)], props)
    raw = lambda ctl, n=20: ("raw", ctl, noise(n, n))
    for name, chunks in (("state-resets", [lz(0xE0, (3, 0, 2)), lz(0x80), lz(0xA0), lz(0xC0, (0, 2, 1)), lz(0x80), lz(0xE0, (1, 1, 1)), lz(0xA0)]),
                         ("raw-first", [raw(1), lz(0xC0, (3, 0, 2)), lz(0x80), raw(2), lz(0x80), raw(1, 33), lz(0xE0, (2, 2, 0))]),
                         ("raw-only", [raw(1), raw(2, 7), raw(1, 9), raw(2, 1)])):
        p = K.ChunkProgram("frames/" + name, chunks)
        d, v = p.expand()
        assert v is None
        add("payload/%s" % name, Stream([Block(bytes(d), payload=p.raw(), csize=True, usize=True), Block(C3)], check=4), "ok")
        add("payload/%s/usize+1" % name, Stream([Block(bytes(d), payload=p.raw(), usize=len(d) + 1), Block(C3)], check=4), "bad")
    # ---- trailing bytes: every accepted program again with bytes behind the footer
    for name, x, v, d in list(P):
        if v == "ok":
            P.append(("trailing/" + name, x + b"tail\x00\x00\x00\x00\xfd7zXZ\x00", "ok", d))
    # ---- prefixes
    S = text(400, seed=9)
    small = [("sizes", Stream([Block(S[:150], csize=True, usize=True)])), ("two-blocks", Stream([Block(S[:90]), Block(S[90:130])], check=4)),
             ("sha256", Stream([Block(S[:120])], check=10)),
             ("filtered-then-plain", Stream([Block(S[:100], enc_filters=x86, filters=[(X86, b""), (LZMA2, b"\x10")]), Block(S[100:160])])),
             ("no-blocks", Stream([], check=0))]
    for name, s in small:
        x = s.write()
        for n in range(len(x)):
            P.append(("prefix/%s/%d" % (name, n), x[:n], "short", None))
    _cache["programs"] = P
    return P


def window_programs():
    """-> the same tuples for streams that decode to more than a window of mz_stream_lzma's window mode (128 KiB at the least)
    while staying small themselves: two blocks of 150 000 and 140 000 very repetitive bytes, one framing defect each"""
    if "window" in _cache:
        return _cache["window"]
    P = []
    W1, W2 = (text(1000, 41) * 150)[:150000], (text(900, 42) * 160)[:140000]
    p1, p2 = raw_lzma2(W1), raw_lzma2(W2)
    b1 = lambda **kw: Block(W1, payload=p1, **kw)
    b2 = lambda **kw: Block(W2, payload=p2, **kw)

    def add(name, s, verdict):
        P.append(("window/" + name, s.write(), verdict, s.data()))

    for cid in (0, 1, 4):
        add("ok/check-%d" % cid, Stream([b1(csize=True, usize=True), b2()], check=cid), "ok")
        add("check-%d/second-header-reserved-bit" % cid, Stream([b1(), b2(flags_or=0x08)], check=cid), "bad")
        add("check-%d/index-count+1" % cid, Stream([b1(), b2()], check=cid, count=3), "bad")
    for d in (1, -1):
        add("csize%+d" % d, Stream([b1(csize=len(p1) + d), b2()]), "bad")
        add("usize%+d" % d, Stream([b1(usize=len(W1) + d), b2()]), "bad")
        add("second-block/csize%+d" % d, Stream([b1(), b2(csize=len(p2) + d)], check=4), "bad")
        add("second-block/usize%+d" % d, Stream([b1(), b2(usize=len(W2) + d)], check=4), "bad")
    add("csize-2^63-1", Stream([b1(csize=V63), b2()]), "bad")
    add("second-block/csize-2^63-4", Stream([b1(), b2(csize=V63 - 3)]), "bad")
    add("csize-half", Stream([b1(csize=len(p1) // 2), b2()]), "bad")
    add("csize-12", Stream([b1(csize=12), b2()]), "bad")
    add("csize-3", Stream([b1(), b2(csize=3)]), "bad")
    add("usize-100000", Stream([b1(usize=100000), b2()]), "bad")
    add("second-block/usize-7", Stream([b1(), b2(usize=7)]), "bad")
    add("block-padding", Stream([b1(bpad_byte=1 if len(p1) % 4 else 0, check=None if len(p1) % 4 else 1), b2()]), "bad")
    add("check-wrong", Stream([b1(check=0x20), b2()], check=4), "bad")
    add("second-block/check-wrong", Stream([b1(), b2(check=0x20)], check=1), "bad")
    add("second-block/header-crc", Stream([b1(), b2(hcrc_xor=4)]), "bad")
    add("index-crc", Stream([b1(), b2()], index_crc_xor=1), "bad")
    for extra in ([], [Block(b"x")], [Block(text(200, 43))]):                # (whichever leaves index padding to spoil)
        recs = Stream([b1(), b2()] + extra).true_records()
        if -(2 + sum(len(vli(v)) for r in recs for v in r)) % 4:
            add("index-padding", Stream([b1(), b2()] + extra, ipad_byte=0x40), "bad")
            break
    ilo, ihi = Stream([b1(), b2()]).layout()[1]["index"][0]
    add("footer-backward+1", Stream([b1(), b2()], backward=(ihi - ilo + 4) // 4), "bad")
    add("footer-flags", Stream([b1(), b2()], foot_flags=b"\x00\x04"), "bad")
    _cache["window"] = P
    return P


STATUS = {"ok": OK, "bad": DATA_ERROR, "short": BUF_ERROR}


def verdicts(which=programs):
    """-> [(name, stream, status, data, in_used)] as liblzma judged them (data and in_used: accepted streams only)"""
    key = ("verdicts", which.__name__)
    if key not in _cache:
        V = []
        for name, x, v, d in which():
            st, used, out = judge(x)
            V.append((name, x, st, out if st == OK else None, used))
        _cache[key] = V
    return _cache[key]


def partials(which=programs):
    """-> {name: the bytes liblzma had handed out} of the programs it wants more input for (a cut filtered block: what its
    filter chain had finished)"""
    key = ("partials", which.__name__)
    if key not in _cache:
        _cache[key] = {name: out for name, x, v, d in which() for st, used, out in [judge(x)] if st == BUF_ERROR}
    return _cache[key]


# ---- re-sealed mutations --------------------------------------------------------------------------------------------------
ZONES = ("flags", "header1", "header2", "index", "footer")
ZONE_DRAW = ("flags",) * 2 + ("header1", "header2") * 3 + ("index", "footer")  # (the headers hold the fields with more than one valid value)
RESEAL_CHECKS = (0, 1, 4, 10, 7)


def _bases():
    if "bases" not in _cache:
        R = text(1500, seed=31)
        out = []
        for cid in RESEAL_CHECKS:
            x, z = Stream([Block(R[:700], csize=True, usize=True), Block(R[700:])], check=cid).layout()
            zones = {"flags": z["flags"][0], "header1": z["header"][0], "header2": z["header"][1], "index": z["index"][0], "footer": z["footer"][0]}
            out.append((x, zones))
        _cache["bases"] = out
    return _cache["bases"]


def reseal(x, zones):
    """recompute the stream flags', the two block headers', the index's and the footer's CRC-32 of a mutated image, each
    where the parser will look for it (a header's size byte and the index's record count may be among the mutated bytes)"""
    x = bytearray(x)
    x[8:12] = crc32le(x[6:8])
    for k in ("header1", "header2"):
        h = zones[k][0]
        hs = (x[h] + 1) * 4
        if x[h] and h + hs <= len(x):
            x[h + hs - 4:h + hs] = crc32le(x[h:h + hs - 4])
    ipos, lim = zones["index"][0], len(x) - 12
    p, ok = ipos + 1, True
    r = read_vli(x, p, lim)
    if r and r[0] <= 64:
        p = r[1]
        for _ in range(2 * r[0]):
            r = read_vli(x, p, lim)
            if not r:
                ok = False
                break
            p = r[1]
    else:
        ok = False
    end = ipos + ((p - ipos + 3) & ~3) if ok else zones["index"][1]
    if end + 4 <= len(x):
        x[end:end + 4] = crc32le(x[ipos:end])
    x[-12:-8] = crc32le(x[-8:-2])
    return bytes(x)


def _filter_ids(x, h):
    """the filter ids a parser reads in the block header at h (as far as it is well-formed)"""
    hs = (x[h] + 1) * 4
    hend, p, fl = h + hs - 4, h + 2, x[h + 1]
    ids = []
    if hend > len(x):
        return ids
    for bit in (0x40, 0x80):
        if fl & bit:
            r = read_vli(x, p, hend)
            if not r:
                return ids
            p = r[1]
    for _ in range((fl & 3) + 1):
        r = read_vli(x, p, hend)
        r2 = r and read_vli(x, r[1], hend)
        if not r2:
            return ids
        ids.append(r[0])
        p = r2[1] + r2[0]
    return ids


def resealed(seed, n):
    """-> [(name, stream, zones hit)]: one or two framing bytes of a two-block base (blocks of 700 and 800 bytes, both size
    fields in the first header; check ids 0, 1, 4, 10 and 7 in turn) changed -- a bit flipped, a random byte, 0, 0x80, 0xFF,
    plus or minus one -- in the stream flags, a block header, the index or the footer, then re-sealed; every other change to
    the stream flags is made to the footer's copy as well (the second change), so that check ids other than the encoder's
    are decoded and not only refused.  Filter ids from 0x0A
    up (ARM64, RISC-V: known to newer liblzma builds only) are kept out: a mutant whose headers name one is drawn again."""
    rnd = random.Random(seed)
    bases = _bases()
    out = []
    while len(out) < n:
        x0, zones = bases[len(out) % len(bases)]
        x = bytearray(x0)
        hit = []
        for _ in range(rnd.choice((1, 1, 2))):
            zn = rnd.choice(ZONE_DRAW)
            lo, hi = zones[zn]
            at = rnd.randrange(lo, hi)
            op = rnd.choice((0, 0, 0, 1, 2, 3, 4, 5, 5, 6, 6))  # (the near changes -- a flipped bit, plus or minus one -- more often)
            v = x[at]
            x[at] = (v ^ (1 << rnd.randrange(8)), rnd.randrange(256), 0, 0x80, 0xFF, (v + 1) & 0xFF, (v - 1) & 0xFF)[op]
            hit.append(zn)
            if zn == "flags" and rnd.randrange(2):  # the same change to the footer's copy: flags the two ends agree on
                x[zones["footer"][0] + 4 + at - lo] = x[at]
                hit.append("footer")
                break
        y = reseal(x, zones)
        if y == x0:
            continue
        if any(0x0A <= i != LZMA2 for k in ("header1", "header2") if y[zones[k][0]] for i in _filter_ids(y, zones[k][0])):
            continue
        out.append(("resealed/%d/%d/check%d/%s" % (seed, len(out), y[7] & 15, "+".join(hit)), y, tuple(hit)))
    return out


def resealed_verdicts(seed, n):
    key = ("rv", seed, n)
    if key not in _cache:
        V = []
        for name, x, hit in resealed(seed, n):
            st, used, out = judge(x)
            V.append((name, x, st, out if st == OK else None, used, hit))
        _cache[key] = V
    return _cache[key]
