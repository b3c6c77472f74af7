"""Deterministic synthetic inputs shared by the tests (and mirrored by bench.py).

Corpus C = the English prose shipped with CPython (pydoc_data.topics, ~460 KB): present in
the image both here and on the GPU box, zlib level-6 ratio ~0.31 on 64 KiB slices -- the
stand-in for the "enwik-slice" entries BASELINE.json names (no enwik, no network)."""
import random
import zlib

import numpy as np

from tests.token_programs import _DBASE, _DEXT, _LBASE, _LEXT, fixed_stream, stored_blocks  # noqa: F401  (the writers live there now)


def corpus():
    import pydoc_data.topics as t

    return "".join(t.topics[k] for k in sorted(t.topics)).encode()


def bench_corpus():
    """(bytes, description): the SURVEY 8(d) corpus when oracle/_ref/corpus.bin travelled (built by
    oracle/make_corpus.py from the reference tree), else the CPython prose above."""
    import os

    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "corpus.bin")
    if os.path.exists(p):
        return open(p, "rb").read(), "appnote.txt || appnote.iz.txt || alice29.txt of the reference tree (SURVEY 8d)"
    return corpus(), "CPython's pydoc prose (oracle/_ref/corpus.bin absent)"


_CHAIN = {}


def markov_entries(n_unique, size, seed=3, text=None, jump=0.45):
    """Seeded order-2 word-Markov expansion of the corpus (mandatory for config 4: the corpus is only
    ~470 KB, so 1 MiB entries tiled from slices would repeat inside LZMA's dictionary).  `jump` = probability of leaving
    the chain at a word: 0.45 gives liblzma preset 6 a ratio of ~0.25 on the SURVEY corpus (0.15 without jumps)."""
    rnd = random.Random(seed)
    src = text if text is not None else corpus()
    ck = (len(src), zlib.crc32(src))
    if _CHAIN.get("key") != ck:  # the chain of one corpus is built once per process (bench.py's workers make one entry per call)
        words = src.split()
        nxt = {}
        for a, b, c in zip(words, words[1:], words[2:]):
            nxt.setdefault((a, b), []).append(c)
        _CHAIN.update(key=ck, nxt=nxt, keys=list(nxt))
    nxt, keys = _CHAIN["nxt"], _CHAIN["keys"]
    out = []
    for _ in range(n_unique):
        a, b = keys[rnd.randrange(len(keys))]
        parts, total = [a, b], len(a) + len(b) + 2
        while total < size + 64:                         # a few words more than needed: the slice below is exactly `size`
            cand = nxt.get((a, b))
            if not cand or rnd.random() < jump:          # dead end, or a jump: keeps phrases short enough for an LZMA ratio of ~0.25
                a, b = keys[rnd.randrange(len(keys))]
                parts += [a, b]
                total += len(a) + len(b) + 2
                continue
            c = cand[rnd.randrange(len(cand))]
            parts.append(c)
            total += len(c) + 1
            a, b = b, c
        out.append(b" ".join(parts)[:size])
    return out


def slices(n, size, seed=1234):
    c = corpus()
    rnd = random.Random(seed)
    return [c[o:o + size] for o in (rnd.randrange(len(c) - size) for _ in range(n))]


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """Exactly the reference writer's parameters (mz_strm_zlib.c:87: raw, 32 KiB window, memLevel 8)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def edge_payloads():
    """(name, uncompressed bytes, raw deflate bytes) covering the shapes SURVEY 8(d) lists."""
    rnd = np.random.RandomState(7)
    c = corpus()
    cases = []

    def add(name, data, **kw):
        cases.append((name, data, deflate_raw(data, **kw)))

    add("empty", b"")
    add("one_byte", b"x")
    add("run_A_65535", b"A" * 65535)                      # dist=1 overlap, len 258 chains
    add("run_ab", b"ab" * 5000)                           # dist=2 < len
    add("text_64k_l6", c[1000:1000 + 65536])
    add("text_64k_l1", c[5000:5000 + 65536], level=1)
    add("text_64k_l9", c[9000:9000 + 65536], level=9)
    add("text_8k", c[20000:20000 + 8192])
    add("text_fixed", c[30000:30000 + 20000], strategy=zlib.Z_FIXED)
    add("text_huffman_only", c[40000:40000 + 30000], strategy=zlib.Z_HUFFMAN_ONLY)
    add("text_rle", c[50000:50000 + 30000], strategy=zlib.Z_RLE)
    add("random_incompressible", rnd.bytes(70000))        # zlib emits stored blocks
    add("multi_block_300k", c[:300000])                   # several dynamic blocks
    far = rnd.bytes(300)
    add("max_distance", far + rnd.bytes(32768 - 300) + far + c[:500] + far)   # back-refs at distance 32768
    add("binaryish", bytes((i * i >> 3) & 0xFF for i in range(50000)))
    cases.append(("stored_only", c[:70000], stored_blocks(c[:70000])))
    cases.append(("stored_empty", b"", stored_blocks(b"")))
    # a sync-flushed stream: empty stored blocks between dynamic blocks
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    z = co.compress(c[:10000]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(c[10000:25000]) + co.flush(
        zlib.Z_FULL_FLUSH) + co.compress(c[25000:26000]) + co.flush()
    cases.append(("sync_flushed", c[:26000], z))
    return cases


def corruptions(z, seed=3):
    """(name, bytes) malformed variants of a valid raw-deflate stream."""
    rnd = random.Random(seed)
    out = [("truncated_half", z[:len(z) // 2]), ("truncated_1", z[:-1]), ("empty_input", b""),
           ("reserved_btype", bytes([z[0] | 0x06]) + z[1:])]
    for k in range(6):
        i = rnd.randrange(len(z))
        out.append(("flip_%d" % i, z[:i] + bytes([z[i] ^ (1 << rnd.randrange(8))]) + z[i + 1:]))
    i = len(z) // 3
    out.append(("xor55_third", z[:i] + bytes([z[i] ^ 0x55]) + z[i + 1:]))
    return out


# ---- .xz helpers (method 95) -------------------------------------------------------------------------------
def _vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _read_vli(b, p):
    v = s = 0
    while True:
        v |= (b[p] & 0x7F) << s
        s += 7
        p += 1
        if not b[p - 1] & 0x80:
            return v, p


def xz_blocks(x):
    """Split a single-stream .xz image into (check_id, [(block_bytes, unpadded_size, uncompressed_size)])."""
    check = x[7]
    csz = (0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64)[check]
    isize = (int.from_bytes(x[-8:-4], "little") + 1) * 4
    ipos = len(x) - 12 - isize
    n, p = _read_vli(x, ipos + 1)
    recs = []
    for _ in range(n):
        unp, p = _read_vli(x, p)
        usz, p = _read_vli(x, p)
        recs.append((unp, usz))
    pos, out = 12, []
    for unp, usz in recs:
        padded = (unp + 3) & ~3
        out.append((x[pos:pos + padded], unp, usz))
        pos += padded
    assert pos == ipos and csz >= 0
    return check, out


def xz_join(streams):
    """One .xz stream holding every block of the given single-stream images (same check id): a multi-block
    stream like `xz -T` / --block-size writes."""
    check, blocks = None, []
    for x in streams:
        c, b = xz_blocks(x)
        assert check in (None, c)
        check = c
        blocks += b
    flags = bytes([0, check])
    out = b"\xfd7zXZ\x00" + flags + zlib.crc32(flags).to_bytes(4, "little")
    for blk, _, _ in blocks:
        out += blk
    idx = b"\x00" + _vli(len(blocks)) + b"".join(_vli(u) + _vli(s) for _, u, s in blocks)
    idx += b"\x00" * (-len(idx) % 4)
    idx += zlib.crc32(idx).to_bytes(4, "little")
    tail = (len(idx) // 4 - 1).to_bytes(4, "little") + flags
    return out + idx + zlib.crc32(tail).to_bytes(4, "little") + tail + b"YZ"


def xz_cases():
    """(name, data, xz_stream) covering presets, every verified check id, lc/lp/pb variety, stored (uncompressed)
    LZMA2 chunks, multi-chunk and multi-block streams."""
    import lzma

    c = corpus()
    rnd = np.random.RandomState(11)
    noise = rnd.bytes(70000)
    cases = []
    for name, d in (("text100k", c[:100000]), ("empty", b""), ("one", b"a"), ("noise", noise), ("zeros", bytes(300000)),
                    ("text+noise", c[:50000] + noise + c[50000:90000])):
        for chk in (lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64, lzma.CHECK_SHA256):
            cases.append(("%s/check%d" % (name, chk), d, lzma.compress(d, format=lzma.FORMAT_XZ, check=chk, preset=6)))
        for preset in (0, 9):
            cases.append(("%s/preset%d" % (name, preset), d, lzma.compress(d, format=lzma.FORMAT_XZ, preset=preset)))
        for lc, lp, pb, ds in ((0, 2, 0, 4096), (4, 0, 4, 1 << 16), (0, 4, 2, 1 << 20), (1, 3, 1, 1 << 12)):
            f = [{"id": lzma.FILTER_LZMA2, "lc": lc, "lp": lp, "pb": pb, "dict_size": ds}]
            cases.append(("%s/lc%dlp%dpb%d" % (name, lc, lp, pb), d, lzma.compress(d, format=lzma.FORMAT_XZ, filters=f)))
    big = c + c[:200000]          # > 2 MiB would need a bigger corpus; several 64 KiB-compressed chunks is what matters
    cases.append(("multi-chunk", big, lzma.compress(big, format=lzma.FORMAT_XZ, preset=1)))
    parts = [c[:70000], noise[:5000], b"", c[70000:200000]]
    cases.append(("multi-block", b"".join(parts), xz_join([lzma.compress(p, format=lzma.FORMAT_XZ) for p in parts])))
    cases.append(("multi-block-sha", b"".join(parts),
                  xz_join([lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256) for p in parts])))
    cases += xz_filter_cases()
    return cases


def _branch_soup(rnd, n, kind):
    """n bytes of noise in which the branch patterns the BCJ filter `kind` converts are frequent"""
    b = bytearray(rnd.randrange(256) for _ in range(n))
    i = 0
    while i + 16 < n:
        r = rnd.random()
        if kind == "x86" and r < 0.3:
            b[i] = rnd.choice((0xE8, 0xE9))
            b[i + 4] = rnd.choice((0x00, 0xFF, 0x00, 0xFF, rnd.randrange(256)))
            if rnd.random() < 0.3:
                b[i + 1] = rnd.choice((0xE8, 0xE9))       # calls on top of each other: the prev_mask paths
            i += rnd.randrange(1, 9)
        elif kind == "arm" and r < 0.3:
            b[(i & ~3) + 3] = 0xEB
            i += 4
        elif kind == "armthumb" and r < 0.4:
            j = i & ~1
            b[j + 1] = 0xF0 | rnd.randrange(8)
            b[j + 3] = 0xF8 | rnd.randrange(8)
            i += rnd.choice((2, 2, 4, 6))                  # overlapping candidates: the skip-after-a-pair rule
        elif kind == "powerpc" and r < 0.3:
            j = i & ~3
            b[j] = 0x48 | rnd.randrange(4)
            b[j + 3] = (b[j + 3] & ~3) | 1
            i += 4
        elif kind == "sparc" and r < 0.3:
            j = i & ~3
            if rnd.random() < 0.5:
                b[j], b[j + 1] = 0x40, b[j + 1] & 0x3F
            else:
                b[j], b[j + 1] = 0x7F, b[j + 1] | 0xC0
            i += 4
        elif kind == "ia64" and r < 0.5:
            j = i & ~15
            b[j] = (b[j] & 0xE0) | rnd.choice((16, 17, 18, 19, 22, 23, 24, 25, 28, 29))
            for k in range(1, 16):
                if rnd.random() < 0.5:
                    b[j + k] = rnd.choice((0x00, 0x50, 0xA0, 0x0A, 0x28, 0x14, 0x05))
            i += 16
        else:
            i += rnd.randrange(1, 7)
    return bytes(b)


def xz_bad_chain_cases():
    """(name, xz_stream): block headers whose filter chain liblzma refuses (LZMA_OPTIONS_ERROR): a misaligned BCJ start
    offset, an unknown filter id, LZMA2 in front of another filter, Delta last.  Made from valid streams by editing the
    filter flags and re-sealing the header's CRC32."""
    import lzma

    lz2 = {"id": lzma.FILTER_LZMA2, "preset": 1}
    d = corpus()[:3000]

    def reseal(x, edit):
        x = bytearray(x)
        hsize = (x[12] + 1) * 4
        edit(x, 12)
        x[12 + hsize - 4:12 + hsize] = zlib.crc32(bytes(x[12:12 + hsize - 4])).to_bytes(4, "little")
        return bytes(x)

    out = []
    x = lzma.compress(d, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_ARM, "start_offset": 4096}, lz2])
    out.append(("arm start offset 4098", reseal(x, lambda b, h: b.__setitem__(h + 4, 2))))      # id 07, size 04, offset bytes
    x = lzma.compress(d, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_X86}, lz2])
    out.append(("unknown filter 0x0A", reseal(x, lambda b, h: b.__setitem__(h + 2, 0x0A))))
    out.append(("lzma2 in front", reseal(x, lambda b, h: b.__setitem__(slice(h + 2, h + 7), bytes([0x21, 0x01, b[h + 6], 0x04, 0x00])))))
    x = lzma.compress(d, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_DELTA, "dist": 1}, lz2])
    out.append(("delta last", reseal(x, lambda b, h: b.__setitem__(slice(h + 5, h + 8), bytes([0x03, 0x01, 0x00])))))
    return out


def xz_filter_cases():
    """(name, data, xz_stream): .xz blocks whose filter chain has Delta / BCJ filters in front of LZMA2 -- every filter
    liblzma 5.2.5 knows, with and without a start offset, sizes around the filters' unit and look-ahead, more than one
    8 KiB round of the device's unfilter, and chains of two and three filters -- written by liblzma itself."""
    import lzma
    import random

    rnd = random.Random(77)
    bcj = (("x86", lzma.FILTER_X86, 1), ("powerpc", lzma.FILTER_POWERPC, 4), ("ia64", lzma.FILTER_IA64, 16),
           ("arm", lzma.FILTER_ARM, 4), ("armthumb", lzma.FILTER_ARMTHUMB, 2), ("sparc", lzma.FILTER_SPARC, 4))
    lz2 = {"id": lzma.FILTER_LZMA2, "preset": 1}
    cases = []
    for kind, fid, align in bcj:
        for k, n in enumerate((0, 3, 4, 5, 15, 16, 17, 5000, 70000)):
            f = {"id": fid}
            if k % 2:
                f["start_offset"] = align * rnd.randrange(1, 1 << 20)
            d = _branch_soup(rnd, n, kind)
            cases.append(("filter/%s/%d" % (kind, n), d, lzma.compress(d, format=lzma.FORMAT_XZ, filters=[f, lz2])))
        d = bytes(rnd.getrandbits(8) for _ in range(40000)) + _branch_soup(rnd, 60000, kind)
        cases.append(("filter/%s/100k-crc64" % kind, d, lzma.compress(d, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64,
                                                                     filters=[{"id": fid, "start_offset": align * 777}, lz2])))
    for dist in (1, 2, 3, 4, 7, 63, 64, 65, 255, 256):
        n = rnd.choice((0, 1, dist, dist + 1, 3000, 50000))
        d = bytes((rnd.randrange(256) if rnd.random() < 0.1 else (i * 3) & 255) for i in range(n))
        cases.append(("filter/delta%d/%d" % (dist, n), d,
                      lzma.compress(d, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_DELTA, "dist": dist}, lz2])))
    d = _branch_soup(rnd, 40000, "x86")
    cases.append(("filter/x86+delta4", d, lzma.compress(d, format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256, filters=[
        {"id": lzma.FILTER_X86}, {"id": lzma.FILTER_DELTA, "dist": 4}, lz2])))
    cases.append(("filter/delta1+delta2+arm", d, lzma.compress(d, format=lzma.FORMAT_XZ, filters=[
        {"id": lzma.FILTER_DELTA, "dist": 1}, {"id": lzma.FILTER_DELTA, "dist": 2}, {"id": lzma.FILTER_ARM}, lz2])))
    return cases


def long_code_payloads(size=200000):
    """(name, data, raw_deflate): streams whose dynamic Huffman codes reach 13-15 bits and use many symbols: long codes
    from zlib's own Huffman construction (zlib Z_HUFFMAN_ONLY / level 9 on data with geometric byte statistics, all 256
    byte values present), which fill a fraction of the decoder's second-level literal/length table -- the code that fills
    it to its capacity is in the `sets` family of tests/header_programs.py.  size: bytes drawn (the rare symbols are the
    512 bytes behind them, so the code lengths stay as long at a tenth of the default)."""
    out = []
    for seed, ratio in ((1, 0.5), (2, 0.6), (3, 0.7), (4, 0.8)):
        rnd = np.random.RandomState(seed)
        p = ratio ** np.arange(256, dtype=np.float64)
        p /= p.sum()
        perm = rnd.permutation(256)
        d = perm[rnd.choice(256, size=size, p=p)].astype(np.uint8).tobytes()
        d += bytes(range(256)) * 2                      # every byte value at least twice
        for strat, nm in ((zlib.Z_HUFFMAN_ONLY, "huff"), (zlib.Z_DEFAULT_STRATEGY, "l9")):
            out.append(("geom%.1f/%s" % (ratio, nm), d, deflate_raw(d, level=9, strategy=strat)))
    return out


# ---- streams made by hand: fixed-Huffman blocks of chosen tokens (zlib never emits distance 32768) ----------------------

def hand_made():
    rnd = np.random.RandomState(21)
    lit = [int(v) for v in rnd.randint(0, 256, size=32768)]
    c = corpus()
    cases = []
    cases.append(("ends_in_258_match", fixed_stream(list(c[:700]) + [(258, 300)])))
    cases.append(("ends_in_258_run", fixed_stream([65, (258, 1)])))
    cases.append(("runs_258", fixed_stream([66] + [(258, 1)] * 40)))
    cases.append(("dist_32768", fixed_stream(lit + [(258, 32768), (3, 32768), 7, (100, 32768)])))
    cases.append(("dist_32768_then_258_end", fixed_stream(lit + [5] * 9 + [(258, 32768)])))
    return cases


# ---- wave reuse: a table of small, unique streams with their reference results ---------------------------------------
_REUSE = {}


def _kind(name, z, cap, st, used, out, max_out=-1, refused=None):
    """one decoder kind: the stream, the room it is given, and what the reference makes of it"""
    return dict(name=name, z=z, cap=cap, max_out=max_out, status=st, in_used=used, out_len=len(out), data=out, crc=zlib.crc32(out),
                refused=refused, long=cap > 32768)


def reuse_kinds():
    """{"deflate" | "lzma" | "xz": [kind, ...], "enc": [(name, bytes), ...]}: what tests/test_kernel_emul.py runs in pairs through
    one wave's state and tests/test_gpu_wave_reuse.py draws its launches from.  A decoder kind is a dict: name, z (the stream),
    cap (out_cap), max_out, refused (None for a good kind, else the status the kind is named after), long (more than 32 KiB
    of room: the kinds a launch of thousands of entries takes one entry in 97 from) and the reference result: status, in_used, out_len, crc from the oracle restatement, data = the bytes (zlib /
    lzma say the same of every good kind: test_kernel_emul.test_reuse_kinds_are_what_they_claim).  Built once per process;
    nobody changes it."""
    if _REUSE:
        return _REUSE
    import lzma

    import oracle
    from tests.test_oracle import INCOMPLETE_DISTANCE_SET, _zip_lzma

    c = corpus()
    rnd = np.random.RandomState(97)
    noise = rnd.bytes(3000)

    # DEFLATE
    def dk(name, z, cap, refused=None):
        st, used, out = oracle.inflate_raw(z, cap)
        return _kind(name, z, cap, st, used, out, refused=refused)

    def good(name, data, z):
        return dk(name, z, len(data))

    dyn = deflate_raw(c[20000:23000])
    hm = dict(hand_made())
    dist_data = zlib.decompress(hm["dist_32768"], -15)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    flushed = b"".join(co.compress(c[40000 + 90 * i:40000 + 90 * (i + 1)]) + co.flush(zlib.Z_FULL_FLUSH if i % 3 == 2 else zlib.Z_SYNC_FLUSH)
                       for i in range(30)) + co.flush()
    D = [good("empty", b"", deflate_raw(b"")), good("one_byte", b"x", deflate_raw(b"x")),
         good("stored", c[:3000], stored_blocks(c[:3000], block=1000)),
         good("fixed", c[30000:32000], deflate_raw(c[30000:32000], strategy=zlib.Z_FIXED)),
         good("dynamic_short", c[20000:23000], dyn)]
    D += [good("long_codes/" + n, d, z) for n, d, z in long_code_payloads(20000)]
    D += [good("flushed_blocks", c[40000:40000 + 2700], flushed), good("dist_32768", dist_data, hm["dist_32768"]),
          good("runs_258", b"B" * (1 + 258 * 40), hm["runs_258"]),
          good("text_64k_l9", c[9000:9000 + 65536], deflate_raw(c[9000:9000 + 65536], level=9)),
          good("noise", noise, deflate_raw(noise))]
    dh = deflate_raw(bytes(range(256)) * 4 + c[:1500])          # every literal in use: a long dynamic header
    stored = stored_blocks(c[:3000], block=1000)
    D += [dk("cut_mid_block", dyn[:len(dyn) // 2], 4000, -5), dk("cut_in_dynamic_header", dh[:20], 4000, -5),
          dk("cut_stored", stored[:1500], 4000, -5),
          dk("invalid_code", fixed_stream(list(c[:300]) + [286] + list(c[300:400])), 4000, -3),        # (symbol 286 has a code and no meaning)
          dk("stored_bad_nlen", stored[:1005] + bytes([stored[1005], stored[1006], stored[1007] ^ 1]) + stored[1008:], 4000, -3),
          dk("far0", fixed_stream([(258, 1), 65, 66]), 4000, -3),
          dk("far100", fixed_stream(list(c[:100]) + [(258, 32768), 67]), 4000, -3),
          dk("incomplete_distance_set_0", INCOMPLETE_DISTANCE_SET[0], 4000, -3),
          dk("incomplete_distance_set_1", INCOMPLETE_DISTANCE_SET[1], 26000, -3),       # (25 286 bytes of matches come first)
          dk("out_cap_one_short", dyn, 3000 - 1, -200)]

    # LZMA (ZIP method 14)
    def lk(name, z, cap, max_out=-1, refused=None):
        st, used, out = oracle.lzma_zip_decode(z, cap, max_out)
        if refused == -5 and st == -3:
            # The restatement answers what mz_stream_lzma_read answers, and that folds liblzma's LZMA_BUF_ERROR (the input ends
            # inside a valid stream) into MZ_DATA_ERROR (mz_strm_lzma.c:236).  The device says which of the two it was
            # (lzma_entry.inc `finish`: -5), as liblzma does; test_reuse_kinds_are_what_they_claim holds this kind against
            # liblzma: no error, and no end of stream either.
            st = -5
        return _kind(name, z, cap, st, used, out, max_out=max_out, refused=refused)

    def alone(d, **f):
        raw = lzma.compress(d, format=lzma.FORMAT_ALONE, filters=[dict(id=lzma.FILTER_LZMA1, preset=6, **f)])
        return bytes([5, 2, 5, 0]) + raw[:5] + raw[13:]

    d = c[50000:53000] + bytes(range(256)) * 3
    Z = [lk("lc%dlp%dpb%d" % p, alone(d, lc=p[0], lp=p[1], pb=p[2]), len(d), len(d))
         for p in ((4, 0, 2), (3, 1, 2), (0, 4, 0), (2, 2, 4), (1, 3, 1), (0, 0, 0), (3, 0, 4), (3, 0, 2))]
    text = _zip_lzma(c[60000:64000])
    Z += [lk("run", _zip_lzma(b"A" * 4000), 4000, 4000), lk("text", text, 4000), lk("noise", _zip_lzma(noise), 3000, 3000),
          lk("max_out_clamp", text, 4000, 2500)]
    bad = None
    for seed in range(200):              # a stream whose first packet is a match (rep0 beyond the empty dictionary)
        cand = text[:9] + b"\x00" + np.random.RandomState(seed).bytes(40)
        r = oracle.lzma_zip_decode(cand, 4000, -1)
        if r[0] == -3 and r[2] == b"":
            bad = cand
            break
    assert bad is not None
    props = bytearray(text)
    props[4] = 4 + 9 * 1 + 45 * 2        # lc 4, lp 1
    Z += [lk("first_packet_match", bad, 4000, refused=-3), lk("cut", text[:len(text) // 2], 4000, refused=-5),
          lk("lc_plus_lp_5", bytes(props), 4000, refused=-3), lk("first_coder_byte", text[:9] + b"\x01" + text[10:], 4000, refused=-3),
          lk("out_cap_one_short", text, 3999, refused=-200)]

    # .xz (method 95)
    def xk(name, x, cap, max_out=-1, refused=None):
        st, used, out = oracle.xz_decode(x, cap, max_out)
        return _kind(name, x, cap, st, used, out, max_out=max_out, refused=refused)

    every = {n: (dd, x) for n, dd, x in xz_cases()}            # (xz_filter_cases() is part of it)
    X = []
    for n in ("one/check0", "one/check1", "one/check4", "one/check10", "empty/check1", "one/lc0lp4pb2", "filter/x86/5000", "filter/arm/17",
              "filter/ia64/5000", "filter/delta1+delta2+arm", "multi-block"):
        dd, x = every[n]
        X.append(xk(n, x, len(dd)))
    t4 = c[70000:74000]
    for chk in (lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64, lzma.CHECK_SHA256):
        X.append(xk("text4k/check%d" % chk, lzma.compress(t4, format=lzma.FORMAT_XZ, check=chk, preset=6), len(t4)))
    parts = [c[1000:2500], noise[:700], b"", c[3000:4000]]
    X.append(xk("multi-block-small-sha", xz_join([lzma.compress(p, format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256) for p in parts]), 3200))
    X.append(xk("text4k/lc1lp3", lzma.compress(t4, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_LZMA2, "lc": 1, "lp": 3, "pb": 1, "dict_size": 4096}]), len(t4)))
    X.append(xk("max_out_clamp", X[12]["z"], len(t4), 2500))
    good_x = lzma.compress(t4, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=6)
    flip = bytearray(good_x)
    flip[-12 - 8 - 8 + 3] ^= 0x40          # inside the block's CRC-64 (index 8 bytes, footer 12)
    X += [xk("bad_chain/" + n, x, 4000, refused=-3) for n, x in xz_bad_chain_cases()]
    X += [xk("cut", good_x[:len(good_x) // 2], 4000, refused=-5), xk("check_flipped", bytes(flip), 4000, refused=-3),
          xk("out_cap_one_short", good_x, len(t4) - 1, refused=-200)]

    # encoder inputs
    E = [("empty", b""), ("one_byte", b"q"), ("run_258", b"z" * 258), ("text", c[80000:83000]), ("noise", noise[:2000]),
         ("text+noise", c[90000:91500] + noise[:1000] + c[91500:92000]), ("text_64k", c[100000:100000 + 65536]),
         ("text_70000", c[200000:270000])]
    _REUSE.update(deflate=D, lzma=Z, xz=X, enc=E)
    return _REUSE


# ---- encoder inputs that put the window bound, the block choice and the piece framing under load ----------------------
_ECHO = {}


def echo_cases(window_log2):
    """[(name, data, period)]: inputs for a raw-DEFLATE ENCODER told to keep its matches within 2^window_log2 - 262 bytes
    (zlib's MAX_DIST, include/mzhip.h).  "echo/P": a seeded random block R of P bytes, R again, and 300 bytes of R a third
    time (n = 2 P + 300), for P just below, at and just above both 2^w - 262 and 2^w.  R is random, so the only source of the
    second copy lies exactly P back: an encoder that may take it (P <= 2^w - 262) should, one that may not has literals
    left.  period = P for these, None for the rest: "text_echo" = 3 x 2^w bytes of the bench corpus (matches at every
    distance on offer, the far ones tempting), and a run, a short period and two-symbol noise of at most 4 KiB, where a lazy
    rule and matches handed from one position to the next are busiest.  For w = 15 the largest echo (65 838 bytes) crosses the
    encoder's 64 KiB block.  Built once per process; nobody changes it."""
    w = window_log2
    if w in _ECHO:
        return _ECHO[w]
    max_dist = (1 << w) - 262
    cases = []
    for k, p in enumerate((max_dist - 1, max_dist, max_dist + 1, (1 << w) - 1, 1 << w, (1 << w) + 1)):
        r = np.random.RandomState(1000 * w + k).bytes(p)
        cases.append(("echo/%d" % p, r + r + r[:300], p))
    text, _ = bench_corpus()
    cases.append(("text_echo", (text * (3 * (1 << w) // len(text) + 1))[:3 * (1 << w)], None))
    rnd = np.random.RandomState(1000 * w + 99)
    cases.append(("run", b"r" * 4096, None))
    cases.append(("period7", (rnd.bytes(7) * 600)[:4093], None))
    cases.append(("two_symbols", bytes(rnd.randint(0, 2, size=4095, dtype=np.uint8) + 97), None))
    _ECHO[w] = cases
    return cases


def incompressible_cases():
    """[(name, data)]: seeded random bytes of 1, 65535, 65536, 65537 and 131071 bytes: no code shortens them, so a DEFLATE
    encoder that takes the cheapest block kind stores them, 65535 bytes (the most LEN can say) to a block."""
    if "noise" not in _ECHO:
        _ECHO["noise"] = [("noise/%d" % n, np.random.RandomState(7000 + k).bytes(n)) for k, n in enumerate((1, 65535, 65536, 65537, 131071))]
    return _ECHO["noise"]


def lzma_echo_cases(far):
    """[(name, data, period)]: inputs for the LZMA ENCODER (K6), whose matches reach back 32 KiB in a stream of one 64 KiB
    block and far - 1 bytes (far = its history_bytes()) in a longer one, and whose packets never cross a multiple of 64 KiB.
    period = (D, second): the bytes from `second` on repeat what lies exactly D back, and nothing else does -- an encoder
    that may take that echo should, one that may not has literals left -- or None.
      "near/P"  r + r[:65536 - P], r = P random bytes: one block, the echo at the reach of a one-block stream and one short
                of it; "near/32769": the far layout below in 36869 bytes, one byte beyond that reach;
      "far/D"   R + zeros + R + b"tail", R = 4096 random bytes, the second R exactly D back: at and around one block, with
                the second R across a seam of the parse (2 and 16 blocks, less 2000 and 1999), at 1 MiB, at far - 1 (taken)
                and at far and far + 1 (not taken).  The filler is zeros so that the chain pass's table stays clean: all-zero
                positions share one bucket, and R's second copy finds its first directly, whatever the chain depth;
      structure only: nothing, one byte, runs of 300, 65536 and 65537 bytes, text of 200000 bytes and of one block less one,
                exactly, plus one, and a block of noise in front of text (the .xz writer stores it).
    The three far-sized cases are 8.4 MB each.  Built once per process; nobody changes it."""
    key = ("lzma", far)
    if key in _ECHO:
        return _ECHO[key]
    c = corpus()
    cases = []
    for k, p in enumerate((32767, 32768)):
        r = np.random.RandomState(8100 + k).bytes(p)
        cases.append(("near/%d" % p, r + r[:65536 - p], (p, p)))
    R = np.random.RandomState(8200).bytes(4096)
    far_layout = lambda d: R + bytes(d - 4096) + R + b"tail"
    cases.append(("near/32769", far_layout(32769), (32769, 32769)))
    for d in (65536, 65537, 2 * 65536 - 2000, 2 * 65536 - 1999, 16 * 65536 - 2000, 1 << 20, far - 1, far, far + 1):
        cases.append(("far/%d" % d, far_layout(d), (d, d)))
    noise = np.random.RandomState(8300).bytes(65536)
    for name, d in (("empty", b""), ("one", b"a"), ("run/300", b"r" * 300), ("run/65536", b"r" * 65536), ("run/65537", b"r" * 65537),
                    ("text/200000", c[:200000]), ("text/65535", c[:65535]), ("text/65536", c[:65536]), ("text/65537", c[:65537]),
                    ("noise+text", noise + c[:1000])):
        cases.append((name, d, None))
    _ECHO[key] = cases
    return cases
