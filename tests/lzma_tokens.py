"""A packet walker for LZMA1, LZMA2 and .xz: what a stream is made of, not only what it decodes to.

The LZMA encoder's tests need to MEASURE what include/mzhip.h and lzma_enc_core.h promise of K6's output -- how far back a
match reaches and that it reaches that far, that no packet crosses a 64 KiB seam of the parse, the header and its dictionary,
the one end marker, a coder that ends on its last byte, the LZMA2 chunk headers.  A decoder cannot tell: it accepts any
distance its dictionary holds.  walk_lzma() reads a stream packet by packet and returns its packets, its bytes, the input it
used and the coder's last word; it raises LzmaError on everything the format forbids.  The reader itself is
tests/lzma_tokens.cpp, written from the LZMA specification and the .xz format description alone (it shares no code and no
tables with the decoders or the encoder of this project, the oracle restatement or tests/lzma_packets.py);
this module compiles it with g++ on first use, as tests/deflate_tokens.py does, and needs neither a GPU nor a network.
tests/test_lzma_tokens.py holds it against the packet programs of tests/lzma_packets.py and against liblzma's own output.

Throughput, measured on one CPU core with the bytes reconstructed: 200 000 bytes of the test corpus as liblzma preset 6 codes
them (22 700 packets) and as K6's four-way class does (22 200 packets) at 29 - 30 MB of output per second, 7 ms each; K6's
stream for an 8.4 MB echo case of synth.lzma_echo_cases (30 900 packets, almost all of it long copies) at 275 MB/s, 0.03 s.
The device grid of tests/test_gpu_lzma_tokens.py is about 40 MB of output per launch: a fraction of a second of walking."""
import collections
import ctypes as C
import hashlib
import os
import subprocess
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "lzma_tokens.cpp")

LITERALS, MATCH, REP0, REP1, REP2, REP3, SHORTREP, EOS = range(8)
KIND_NAMES = ("literals", "match", "rep0", "rep1", "rep2", "rep3", "shortrep", "eos")
BLOCK = 65536            # the encoder's parse block = one LZMA2 chunk of its .xz writer (deflate_core.h MZ_DEF_BLOCK)
NEAR = 32768             # what a stream of one block looks back over (lzma_enc_core.h mz_lz_tokenize)
MINMATCH, MAXMATCH = 4, 273           # MZ_DEF_MINMATCH .. the longest length LZMA codes
FAR_MINLEN = 5           # lzma_enc_core.h MZ_LZE_FAR_MINLEN

Walk = collections.namedtuple("Walk", "packets rep_hit data used eos code")
Walk.__doc__ = """packets: int64 array [n, 4] of (out_pos, kind, length, distance) -- kind as the constants above; a run of literals
is ONE row whose length is their count (distance 0); the end marker's distance is 2^32; out_pos counts from the stream's own
first byte.  rep_hit: int8 [n], for a MATCH row the index of the repeat distance (as it stood in front of the packet) that the
coded distance equals, else -1.  data: the bytes the stream stands for.  used: input bytes the coder read, its first five
included.  eos: whether an end marker was read.  code: the range decoder's `code` behind the last packet."""
Chunk = collections.namedtuple("Chunk", "control usize csize props stored first_packet npackets out_start in_start code")
Walk2 = collections.namedtuple("Walk2", "chunks packets rep_hit data used")
Walk2.__doc__ = """chunks: [Chunk] (props: the properties byte or -1; in_start: offset of the chunk's payload in the input; code: the
coder's last word); packets / rep_hit / data as Walk, positions counted over the whole chunk sequence; used: input bytes, the
end byte 0x00 included."""
XzBlock = collections.namedtuple("XzBlock", "header_size filter_ids dict_byte dict_size compressed_size uncompressed_size body_start walk unpadded_size")
XzWalk = collections.namedtuple("XzWalk", "check blocks data used")


class LzmaError(ValueError):
    """the stream is not valid LZMA / LZMA2 / .xz; the message names the rule, the input byte, the output byte and the packet;
    out_pos = bytes the stream had produced when the rule was broken (None for a container error)"""

    def __init__(self, msg, out_pos=None):
        ValueError.__init__(self, msg)
        self.out_pos = out_pos


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    with open(_SRC, "rb") as f:
        tag = hashlib.sha1(f.read()).hexdigest()[:12]
    name = "liblzma_tokens_%s.so" % tag
    out = os.path.join(ROOT, "tests", "emul", "_build")
    try:
        os.makedirs(out, exist_ok=True)
        if not os.access(out, os.W_OK):
            raise OSError
    except OSError:
        out = os.path.join(tempfile.gettempdir(), "lzma_tokens_%d" % os.getuid())
        os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    if not os.path.exists(so):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", _SRC, "-o", tmp], check=True)
        os.replace(tmp, so)          # (two processes that build at once both end with a whole file)
    L = C.CDLL(so)
    L.lt_lzma.restype = C.c_void_p
    L.lt_lzma.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int64, C.c_char_p, C.c_uint64]
    L.lt_lzma2.restype = C.c_void_p
    L.lt_lzma2.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64]
    L.lt_error.restype = C.c_int
    L.lt_error.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.lt_counts.restype = None
    L.lt_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.lt_fetch.restype = None
    L.lt_fetch.argtypes = [C.c_void_p] * 5
    L.lt_free.restype = None
    L.lt_free.argtypes = [C.c_void_p]
    _lib = L
    return L


def dict_limit(dict_size, liblzma=False):
    """how far back a distance may reach under a header that states dict_size: the specification's decoder takes at least
    4096; liblzma: what liblzma 5.2 allocates (a multiple of 16 above that), which is what tests/lzma_packets.py's
    programs were written against"""
    d = max(int(dict_size), 4096)
    return (d + 15) & ~15 if liblzma else d


def _collect(L, h):
    """-> (counts, packets, rep_hit, bytes, chunk rows); raises LzmaError"""
    try:
        c = (C.c_uint64 * 8)()
        L.lt_counts(h, c)
        msg = C.create_string_buffer(256)
        if L.lt_error(h, msg, 256):
            raise LzmaError(msg.value.decode(), out_pos=int(c[1]))
        packets = np.zeros((c[0], 4), dtype=np.int64)
        hit = np.zeros(c[0], dtype=np.int8)
        out = np.zeros(c[1], dtype=np.uint8)
        chunks = np.zeros((c[5], 10), dtype=np.int64)
        L.lt_fetch(h, packets.ctypes.data, hit.ctypes.data, out.ctypes.data, chunks.ctypes.data)
    finally:
        L.lt_free(h)
    return [int(v) for v in c], packets, hit, out.tobytes(), chunks


def walk_lzma(z, start, lc, lp, pb, dict_size, usize=None, prefix=None, liblzma=False, exact=True):
    """Read the LZMA1 coder data z[start:] under the given properties -> Walk.

    usize: the size the stream states (then it ends there, with or without bytes left over), None: it ends with its end
    marker.  prefix: bytes that lie in front of the stream's first byte in the same dictionary.  exact (with usize None):
    data behind the end marker, or a coder that does not end on code 0, raises."""
    z = bytes(z)
    L = _load()
    prefix = bytes(prefix) if prefix else b""
    h = L.lt_lzma(z, len(z), start, lc, lp, pb, dict_limit(dict_size, liblzma), -1 if usize is None else usize, prefix, len(prefix))
    c, packets, hit, data, _ = _collect(L, h)
    wk = Walk(packets, hit, data, c[2], bool(c[3]), c[4])
    if exact and usize is None:
        if wk.code != 0:
            raise LzmaError("the range coder does not end on code 0 behind the end marker (code %#x)" % wk.code, out_pos=len(data))
        if start + wk.used != len(z):
            raise LzmaError("data behind the end: the coder used %d of %d bytes" % (wk.used, len(z) - start), out_pos=len(data))
    return wk


def walk_zip14(z, liblzma=False, exact=True):
    """a ZIP method-14 payload (appnote 5.8.8: two version bytes, the size of the properties, the properties) -> (Walk, the
    header's fields as a dict).  liblzma: judge as liblzma 5.2 does where it differs from the specification's decoder -- the
    dictionary rounded up to a multiple of 16 (dict_limit), lc + lp at most 4"""
    z = bytes(z)
    if len(z) < 9:
        raise LzmaError("a method-14 payload has nine header bytes, here are %d" % len(z))
    if z[2:4] != b"\x05\x00":
        raise LzmaError("properties size %d, LZMA1 has five" % int.from_bytes(z[2:4], "little"))
    p = z[4]
    if p > 224:
        raise LzmaError("properties byte %d above 224" % p)
    head = dict(version=(z[0], z[1]), lc=p % 9, lp=p // 9 % 5, pb=p // 45, dict_size=int.from_bytes(z[5:9], "little"))
    if liblzma and head["lc"] + head["lp"] > 4:
        raise LzmaError("properties with lc + lp > 4: the specification codes them, liblzma refuses them")
    return walk_lzma(z, 9, head["lc"], head["lp"], head["pb"], head["dict_size"], liblzma=liblzma, exact=exact), head


def walk_alone(z, liblzma=True):
    """a .lzma file (the properties byte, the dictionary, eight bytes of size, all ones = unknown) -> Walk"""
    z = bytes(z)
    p, ds, n = z[0], int.from_bytes(z[1:5], "little"), int.from_bytes(z[5:13], "little")
    if p > 224:
        raise LzmaError("properties byte %d above 224" % p)
    return walk_lzma(z, 13, p % 9, p // 9 % 5, p // 45, ds, usize=None if n == (1 << 64) - 1 else n, liblzma=liblzma)


def walk_lzma2(body, dict_size, start=0, liblzma=False, exact=False):
    """an LZMA2 chunk sequence body[start:] up to and with its end byte -> Walk2.  exact: bytes behind the end byte raise."""
    body = bytes(body)
    L = _load()
    h = L.lt_lzma2(body, len(body), start, dict_limit(dict_size, liblzma))
    c, packets, hit, data, rows = _collect(L, h)
    if exact and start + c[2] != len(body):
        raise LzmaError("data behind the end byte of the chunk sequence: %d of %d bytes used" % (c[2], len(body) - start), out_pos=len(data))
    return Walk2([Chunk(*(int(v) for v in r)) for r in rows], packets, hit, data, c[2])


def lzma2_dict_size(b):
    """what the one properties byte of the LZMA2 filter states (.xz format 5.3.1)"""
    if b > 40:
        raise LzmaError("LZMA2 dictionary byte %d above 40" % b)
    return 0xFFFFFFFF if b == 40 else (2 | (b & 1)) << (b // 2 + 11)


def _vli(z, p, what):
    v = 0
    for i in range(9):
        if p >= len(z):
            raise LzmaError("the input ends inside %s" % what)
        b = z[p]
        p += 1
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            if b == 0 and i:
                raise LzmaError("%s is not coded in its shortest form" % what)
            return v, p
    raise LzmaError("%s is longer than nine bytes" % what)


_CHECK_BYTES = {0: 0, 1: 4, 4: 8, 10: 32}


def walk_xz(z, liblzma=False):
    """one .xz stream (The .xz File Format 1.0.4) whose blocks have LZMA2 as their only filter -> XzWalk: stream header,
    every block (header with its CRC, the chunk sequence, padding, a CRC-32 check value held against the bytes), the index
    held against the blocks, the footer; nothing may follow it"""
    z = bytes(z)
    if len(z) < 12 or z[:6] != b"\xfd7zXZ\x00":
        raise LzmaError("no .xz stream header")
    flags = z[6:8]
    if flags[0] != 0 or flags[1] not in _CHECK_BYTES:
        raise LzmaError("stream flags %s" % flags.hex())
    if zlib.crc32(flags) != int.from_bytes(z[8:12], "little"):
        raise LzmaError("the stream header's CRC-32")
    check = flags[1]
    p = 12
    blocks, data = [], []
    while True:
        if p >= len(z):
            raise LzmaError("the input ends in front of the index")
        if z[p] == 0:
            break
        hs = (z[p] + 1) * 4
        bh = z[p:p + hs]
        if len(bh) < hs or zlib.crc32(bh[:-4]) != int.from_bytes(bh[-4:], "little"):
            raise LzmaError("block header at %d: its size or its CRC-32" % p)
        bf = bh[1]
        if bf & 0x3C:
            raise LzmaError("block header at %d: reserved flag bits %#x" % (p, bf))
        q = 2
        csz = usz = None
        if bf & 0x40:
            csz, q = _vli(bh, q, "the block's compressed size")
        if bf & 0x80:
            usz, q = _vli(bh, q, "the block's uncompressed size")
        ids, dict_byte = [], None
        for _ in range((bf & 3) + 1):
            fid, q = _vli(bh, q, "a filter id")
            n, q = _vli(bh, q, "a filter's properties size")
            ids.append(fid)
            if fid == 0x21:
                if n != 1:
                    raise LzmaError("LZMA2 filter with %d property bytes" % n)
                dict_byte = bh[q]
            q += n
        if any(bh[q:-4]):
            raise LzmaError("block header at %d: padding that is not zero" % p)
        if ids != [0x21]:
            raise LzmaError("filters %s: this walker reads LZMA2 alone" % [hex(i) for i in ids])
        body = p + hs
        w2 = walk_lzma2(z, lzma2_dict_size(dict_byte), start=body, liblzma=liblzma)
        end = body + w2.used
        if csz is not None and csz != w2.used:
            raise LzmaError("block at %d: compressed size %d stated, %d read" % (p, csz, w2.used))
        if usz is not None and usz != len(w2.data):
            raise LzmaError("block at %d: uncompressed size %d stated, %d made" % (p, usz, len(w2.data)))
        pad = -w2.used % 4
        if any(z[end:end + pad]) or len(z) < end + pad + _CHECK_BYTES[check]:
            raise LzmaError("block at %d: its padding" % p)
        chk = z[end + pad:end + pad + _CHECK_BYTES[check]]
        if check == 1 and int.from_bytes(chk, "little") != zlib.crc32(w2.data):
            raise LzmaError("block at %d: the CRC-32 of its bytes" % p)
        if check == 10 and chk != hashlib.sha256(w2.data).digest():
            raise LzmaError("block at %d: the SHA-256 of its bytes" % p)
        blocks.append(XzBlock(hs, ids, dict_byte, lzma2_dict_size(dict_byte), csz, usz, body, w2, hs + w2.used + len(chk)))
        data.append(w2.data)
        p = end + pad + len(chk)
    i0 = p
    nrec, p = _vli(z, p + 1, "the index's record count")
    if nrec != len(blocks):
        raise LzmaError("the index lists %d blocks, the stream has %d" % (nrec, len(blocks)))
    for b in blocks:
        unp, p = _vli(z, p, "an unpadded size")
        unc, p = _vli(z, p, "an uncompressed size")
        if (unp, unc) != (b.unpadded_size, len(b.walk.data)):
            raise LzmaError("index record (%d, %d), the block has (%d, %d)" % (unp, unc, b.unpadded_size, len(b.walk.data)))
    pad = -(p - i0) % 4
    if any(z[p:p + pad]):
        raise LzmaError("index padding that is not zero")
    p += pad
    if zlib.crc32(z[i0:p]) != int.from_bytes(z[p:p + 4], "little"):
        raise LzmaError("the index's CRC-32")
    p += 4
    foot = z[p:p + 12]
    if len(foot) != 12 or foot[10:] != b"YZ" or foot[8:10] != flags or zlib.crc32(foot[4:10]) != int.from_bytes(foot[:4], "little"):
        raise LzmaError("the stream footer")
    if (int.from_bytes(foot[4:8], "little") + 1) * 4 != p - i0:
        raise LzmaError("the footer's backward size")
    if p + 12 != len(z):
        raise LzmaError("data behind the end: %d bytes behind the stream footer" % (len(z) - p - 12))
    return XzWalk(check, blocks, b"".join(data), p + 12)


# ---- what K6 promises of its output --------------------------------------------------------------------------------------
def _first(rows):
    if not len(rows):
        return ""
    r = rows[0]
    return "output position %d, %s, length %d, distance %d" % (r[0], KIND_NAMES[r[1]], r[2], r[3])


def _echo_len(data, d, second):
    """bytes from `second` on that repeat what lies d back"""
    a = np.frombuffer(data, dtype=np.uint8)
    differ = np.flatnonzero(a[second:] != a[second - d:len(a) - d])
    return int(differ[0]) if len(differ) else len(a) - second


def check_packets(packets, rep_hit, data, far, where=(), period=None, near_cover=False):
    """The packet rules of one parsed stream that stands for `data` (a method-14 stream, or the chunks of one .xz block with
    positions counted over the block); far = the encoder's history_bytes().  See check_encoded."""
    n = len(data)
    m = packets[(packets[:, 1] >= MATCH) & (packets[:, 1] <= SHORTREP)]
    bound = NEAR if n <= BLOCK else far - 1
    short = packets[packets[:, 1] == SHORTREP]
    assert len(short) == 0, (where, "%d short reps; the first: %s" % (len(short), _first(short)))
    bad = m[(m[:, 2] < MINMATCH) | (m[:, 2] > MAXMATCH)]
    assert len(bad) == 0, (where, "%d copies outside %d .. %d bytes; the first: %s" % (len(bad), MINMATCH, MAXMATCH, _first(bad)))
    bad = m[m[:, 3] > m[:, 0]]
    assert len(bad) == 0, (where, "a distance beyond the output: %s" % _first(bad))
    bad = m[m[:, 3] > bound]
    assert len(bad) == 0, (where, "%d of %d copies reach beyond %d; the first: %s" % (len(bad), len(m), bound, _first(bad)))
    bad = m[m[:, 0] // BLOCK != (m[:, 0] + m[:, 2] - 1) // BLOCK]          # seams
    assert len(bad) == 0, (where, "%d copies cover bytes on both sides of a multiple of 65536; the first: %s" % (len(bad), _first(bad)))
    hits = packets[(packets[:, 1] == MATCH) & (rep_hit >= 0)]
    assert len(hits) == 0, (where, "%d match packets code a distance that is a rep distance there; the first: %s" % (len(hits), _first(hits)))
    if period is not None:
        d, second = period
        largest = int(m[:, 3].max()) if len(m) else 0
        at = m[(m[:, 3] == d) & (m[:, 0] >= second)]
        if d <= bound:
            if near_cover:
                assert len(at) >= 1, (where, "no copy at distance %d (largest: %d of %d allowed)" % (d, largest, bound))
            else:
                length = _echo_len(data, d, second)
                covered = int(np.clip(np.minimum(at[:, 0] + at[:, 2], second + length) - at[:, 0], 0, None).sum())
                assert covered >= length - MAXMATCH, (where, "the echo at distance %d is not taken: copies at that distance cover %d of its %d bytes (largest distance: %d of %d allowed)"
                                                      % (d, covered, length, largest, bound))
        else:
            assert len(at) == 0 and largest <= bound, (where, "the echo at distance %d lies beyond the reach (%d): %d copies at it, largest distance %d" % (d, bound, len(at), largest))
    bad = m[(m[:, 3] > NEAR) & (m[:, 2] < FAR_MINLEN)]
    assert len(bad) == 0, (where, "%d copies further than %d back are shorter than %d bytes; the first: %s" % (len(bad), NEAR, FAR_MINLEN, _first(bad)))


def check_encoded(z, data, one_way, far, where=(), period=None, near_cover=False):
    """What include/mzhip.h and lzma_enc_core.h promise of ONE method-14 payload z made from `data`, asserted packet by packet
    -> Walk.  far = mzhip_lzma_encode_history_bytes() / emul_lzma_encode_history_bytes(); one_way: the
    parse class that made it (named in a failure; the rules are the same for both).
      - header: 09 14 05 00 5D, then the dictionary: 65536 for a stream of one block, `far` beyond;
      - the stream stands for exactly `data`; one end marker, the last packet, of length 2; the coder ends on code 0 having
        used every byte of z;
      - every copy is MZ_DEF_MINMATCH .. 273 long; no short rep; no match packet codes one of the four rep distances;
      - every distance <= its output position; <= 32768 in a stream of one block, <= far - 1 otherwise;
      - no copy covers bytes on both sides of a multiple of 65536;
      - no copy further than 32768 back is shorter than MZ_LZE_FAR_MINLEN;
      - period = (D, second) (synth.lzma_echo_cases: the bytes at `second` repeat what lies exactly D back, their only source):
        D within the bound -> copies at distance D that start at `second` or later cover all of the second copy but at most
        273 bytes, one maximal packet of slack (near_cover: at least one such copy -- the 4096-bucket table of a one-block
        stream overwrites most sources); D beyond it -> no copy at that distance, none beyond the bound."""
    z = bytes(z)
    where = tuple(where) + ("one-way" if one_way else "four-way",)
    want_dict = BLOCK if len(data) <= BLOCK else far
    assert z[:5] == bytes([9, 20, 5, 0, 0x5D]), (where, z[:5].hex())
    assert int.from_bytes(z[5:9], "little") == want_dict, (where, "header dictionary %d, expected %d" % (int.from_bytes(z[5:9], "little"), want_dict))
    wk, head = walk_zip14(z, exact=False)
    assert wk.data == data, (where, "the stream stands for other bytes", len(wk.data), len(data))
    p = wk.packets
    eos = np.flatnonzero(p[:, 1] == EOS)
    assert wk.eos and list(eos) == [len(p) - 1] and p[-1, 2] == 2, (where, "end marker", wk.eos, list(eos), len(p), int(p[-1, 2]) if len(p) else None)
    assert wk.code == 0, (where, "the coder ends on code %#x" % wk.code)
    assert 9 + wk.used == len(z), (where, "bytes behind the stream's end", 9 + wk.used, len(z))
    check_packets(p, wk.rep_hit, data, far, where, period, near_cover)
    return wk


def check_xz(z, data, far, where=(), period=None, near_cover=False, lzma2_dict_byte=None):
    """What xz_encode_impl (mzhip_launch.inc) promises of ONE .xz stream z of one block made from `data` -> XzWalk.  lzma2_dict_byte: tests/lzma_packets.py's function (the dictionary byte that states `far`).
      - one filter, LZMA2; the dictionary byte 0x08 for a block of at most one chunk, the byte that states `far` beyond;
      - the chunks cover the input in order, 65536 bytes each but the last; control 0xE0 | size bits (stored: 0x01) for the
        first, 0xC0 | size bits (0x02) behind it; every LZMA chunk brings the properties byte 0x5D;
      - an LZMA chunk has csize <= 65536 and csize < usize (else it had to be stored); its coder ends on code 0 having used
        exactly csize bytes, with no end marker (the walker raises otherwise);
      - the packet rules of check_encoded, positions counted over the block;
      - padding, CRC-32 check value, index and footer as the format says (the walker raises otherwise)."""
    import lzma

    from tests import lzma_packets

    xw = walk_xz(z)
    assert xw.check == 1 and len(xw.blocks) == 1, (where, xw.check, len(xw.blocks))
    assert xw.data == data, (where, "the stream stands for other bytes", len(xw.data), len(data))
    assert lzma.decompress(bytes(z), format=lzma.FORMAT_XZ) == data, where
    check_block(xw.blocks[0], data, far, where, period, near_cover, (lzma2_dict_byte or lzma_packets.lzma2_dict_byte)(far))
    return xw


def check_block(b, data, far, where, period, near_cover, far_byte):
    """the block rules of check_xz for one XzBlock that stands for `data`"""
    chunks = b.walk.chunks
    assert b.filter_ids == [0x21] and b.compressed_size is None and b.uncompressed_size is None, (where, b)
    assert b.dict_byte == (0x08 if len(chunks) <= 1 else far_byte), (where, "dictionary byte %#x for %d chunks" % (b.dict_byte, len(chunks)))
    assert len(chunks) == (len(data) + BLOCK - 1) // BLOCK, (where, len(chunks))
    for i, c in enumerate(chunks):
        us = min(BLOCK, len(data) - i * BLOCK)
        assert c.out_start == i * BLOCK and c.usize == us, (where, i, c)
        if c.stored:
            assert c.control == (0x01 if i == 0 else 0x02), (where, i, hex(c.control))
        else:
            assert c.control == ((0xE0 if i == 0 else 0xC0) | ((us - 1) >> 16)), (where, i, hex(c.control))
            assert c.props == 0x5D, (where, i, hex(c.props))
            assert c.csize <= 65536 and c.csize < c.usize, (where, "chunk %d: %d bytes coded as %d; it had to be stored" % (i, c.usize, c.csize))
            assert c.code == 0, (where, i)
    assert b.walk.data == data, where
    check_packets(b.walk.packets, b.walk.rep_hit, data, far, where, period, near_cover)
