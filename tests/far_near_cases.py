"""The entries of tests/test_far_near_lists_emul.py and tests/test_gpu_far_near_lists.py: token programs (tests/token_programs.py)
around the two lists an emit round of K1 writes (inflate_emit.inc) and the commit copies (inflate_commit.inc).  A piece of a
back-reference -- at most 32 bytes, at offset dw of its chunk, distance dist -- is

    far only    dist >= dw + len    one far entry: fetched from the output buffer;
    near only   dist <= dw          one near entry: copied inside the staging area, in dependency order;
    split       otherwise           a far entry for its first dist - dw bytes and a near entry for the rest.

Where a chunk starts is the kernel's business (the pool, the lanes' groups of records, the window), so no case assumes it: the
offset dw of a match in its chunk is MEASURED with the host emulation's own counters (tests/emul/far_near_main.cpp built with
-DMZ_STATS): the largest distance at which the match makes no far entry.  A case then states the entries it must make --
counted by model() below from the definition above, piece by piece -- and the tests hold the counters of its decode against them.

  edges()      one match of 20 bytes, and one of 258 (nine pieces; the edge inside its third), with dist - dw on, one before and
               one behind both class boundaries;
  all_split()  a chunk in which every piece of a train of 3-byte matches is split, more of them than the pool has room for as two
               entries each (the cut shrinks), with a near-only and a far-only twin of the same bit layout;
  one_kind()   a chunk without a far piece and an entry without a near piece;
  short()      split pieces at distance 1 .. 7: one far byte, which the near part's short-period prologue replicates;
  refused()    a distance that reaches in front of the entry behind a split piece of the same chunk.
zlib judges every stream."""
import ctypes as C
import os
import random
import subprocess

from tests import token_programs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = C.POINTER(C.c_uint8)
_BUILT = {}
PREFIX = 3000            # literals in front of a measured match: some chunks in front of its own
# the kernel's counters (inflate_core.h MZ_STAT) the tests read
BYTES, ENTRIES, NEAR, CHUNKS, SPLIT, NEAR_BATCHES, FAR_BATCHES = 10, 12, 13, 15, 21, 25, 26


def lib(csrc=None, tag="stats"):
    """tests/emul/far_near_main.cpp as a library with the counters on, built when a source is newer than it"""
    if tag not in _BUILT:
        out = os.path.join(ROOT, "tests", "emul", "_build")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "libfar_near_%s.so" % tag)
        inc = csrc or os.path.join(ROOT, "minizip-ng_amd", "csrc")
        srcs = [os.path.join(inc, f) for f in os.listdir(inc)] + [os.path.join(ROOT, "tests", "emul", "far_near_main.cpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
            subprocess.run(["g++", "-O2", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DMZ_STATS", "-I" + inc, "-I" + os.path.join(ROOT, "include"),
                            "-shared", "-fPIC", srcs[-1], "-o", so + ".tmp"], check=True)
            os.replace(so + ".tmp", so)
        L = C.CDLL(so)
        L.fn_inflate.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_ulonglong)]
        L.fn_inflate.restype = C.c_int32
        L.fn_zone.restype = C.c_uint32
        _BUILT[tag] = L
    return _BUILT[tag]


def decode(z, cap, omis=0, L=None):
    """-> (status, out_len, in_used, crc), the cap bytes of the output, the 32 counters, every red zone intact"""
    L = L or lib()
    zone = L.fn_zone()
    src = (C.c_uint8 * (len(z) + 16)).from_buffer_copy(z + bytes(16))
    n = zone + omis + cap + zone
    buf = (C.c_uint8 * n).from_buffer_copy(b"\xA5" * n)
    words, stats = (C.c_uint32 * 4)(), (C.c_ulonglong * 32)()
    ok = L.fn_inflate(src, len(z), buf, omis, cap, words, stats)
    raw = bytes(buf)
    ok = bool(ok) and raw[:zone + omis] == b"\xA5" * (zone + omis) and raw[zone + omis + cap:] == b"\xA5" * zone
    return (C.c_int32(words[0]).value, words[1], words[2], words[3]), raw[zone + omis:zone + omis + cap], list(stats), ok


def model(ln, nfar):
    """(far entries, near entries, split pieces) of a match of ln bytes whose first nfar bytes are older than its chunk"""
    f = n = s = 0
    for o in range(0, ln, 32):
        p = min(32, ln - o)
        pf = min(max(nfar - o, 0), p)
        f += pf > 0
        n += pf < p
        s += 0 < pf < p
    return f, n, s


def _fixed(toks):
    prog = [("fixed", toks, True)]
    return T.encode(prog), T.expand(prog)


def _far_entries(toks):
    z, data = _fixed(toks)
    words, _, s, ok = decode(z, len(data))
    assert ok and words[0] == 0, words
    return s[ENTRIES] - s[NEAR]


def measure_dw(prefix, ln, tail):
    """the offset in its chunk of a match of ln bytes behind `prefix`: the largest distance that makes no far entry (0: the
    match is the first token of its chunk).  The prefix must not be one chunk with the match: then no distance is far."""
    top = min(len(prefix), 32768)
    assert all(isinstance(t, int) for t in prefix) and _far_entries(prefix + [(ln, top)] + tail) > 0
    lo, hi = 0, top           # no far entry at lo (0: by definition), some at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _far_entries(prefix + [(ln, mid)] + tail) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def pieces(toks):
    """pieces of at most 32 bytes the matches of a token list are cut into"""
    return sum((t[0] + 31) // 32 for t in toks if isinstance(t, tuple))


def _case(name, toks, far, near, split, **kw):
    z, data = _fixed(toks)
    return dict(name=name, z=z, data=data, cap=len(data), far=far, near=near, split=split, pieces=pieces(toks), **kw)


def edges():
    """per length 20 and 258: nfar = dist - dw on and next to the class boundaries of the whole match and of its third piece"""
    if "edges" not in _BUILT:
        out = []
        for ln, nfars in ((20, (0, 1, 19, 20, 21)), (258, (0, 1, 63, 64, 65, 95, 96, 97, 257, 258, 300))):
            rnd = random.Random(100 + ln)
            prefix = T._lits(rnd, PREFIX + ln)
            tail = T._lits(rnd, 300)
            dw = measure_dw(prefix, ln, tail)
            assert dw >= 1
            for nfar in nfars:
                f, n, s = model(ln, min(nfar, ln))
                out.append(_case("edges/len%d/nfar%d" % (ln, nfar), prefix + [(ln, dw + nfar)] + tail, f, n, s, dw=dw))
        _BUILT["edges"] = out
    return _BUILT["edges"]


TRAIN = 600              # matches of 3 bytes in the all-split train
LONG = 8                 # matches of 258 bytes in front of it: 2 064 bytes of the chunk in eight records, 72 far entries


def all_split():
    """A chunk in which every piece of the train is split, and which the pool cannot hold at two entries a piece.
    2 900 literals, LONG matches (258, 2500) -- far only wherever they stand --, then TRAIN matches of 3 bytes, match k at
    position p_k with the distance p_k - h + more.  In the chunk that starts at h that is, for more = 1, its offset in the
    chunk plus one: one far byte, two near ones.  Every distance of the train lies in 2049 .. 4096, the two distance codes
    with ten extra bits, so the stream's bit layout is the same for every h and for the twins, and h is found by decoding
    every h of that range and taking the one with the most split pieces.  Per block kind -- a fixed block, and a dynamic one
    whose flat 9-bit literal code fills the second-level tables, so that the pool behind them is smaller -- three entries:
        split   more = 1;
        near    more = 0: near only in that chunk (distance == offset), one entry a piece, far only behind it: its near
                entries are the train's matches the chunk holds when a piece needs one entry;
        far     more = 3: far only everywhere."""
    if "all_split" not in _BUILT:
        out = []
        for kind, opts in (("fixed", None), ("dynamic", {"shape": "flat"})):
            rnd = random.Random(7)
            head, tail = T._lits(rnd, 2900) + [(258, 2500)] * LONG, T._lits(rnd, 300)
            p0 = 2900 + 258 * LONG

            def stream(h, more):
                prog = [(kind, head + [(3, p0 + 3 * k - h + more) for k in range(TRAIN)] + tail, True) + ((opts,) if opts else ())]
                return T.encode(prog), T.expand(prog)

            def splits(h):
                z, data = stream(h, 1)
                return decode(z, len(data))[2][SPLIT]

            # (distances 2049 .. 4096 for more = 0 .. 3; one h less splits the train two far bytes to one near: the larger h is the start)
            h = max(range(p0 + 3 * (TRAIN - 1) + 1 - 4096, p0 - 2048), key=lambda h: (splits(h), h))
            for name, more in (("split", 1), ("near", 0), ("far", 3)):
                z, data = stream(h, more)
                out.append(dict(name="all_split/%s/%s" % (kind, name), z=z, data=data, cap=len(data), lead=p0 - h, pieces=9 * LONG + TRAIN))
        _BUILT["all_split"] = out
    return _BUILT["all_split"]


def one_kind():
    if "one_kind" not in _BUILT:
        rnd = random.Random(8)
        toks, near = T._lits(rnd, 16), 0
        for k in range(150):
            ln = (3, 4, 5, 7, 9, 12, 31, 32, 33, 40)[k % 10] if k % 97 else 258
            toks.append((ln, 1 + (k * 5) % 8))
            near += model(ln, 0)[1]
            if k % 3 == 0:
                toks.append(rnd.randrange(256))
        out = [_case("one_kind/no_far", toks, 0, near, 0, chunks=1)]
        toks, far = T._lits(rnd, 8192), 0
        for k in range(900):
            ln = (3, 4, 6, 11, 32, 33, 64, 65)[k % 8] if k % 113 else 258
            toks.append((ln, 4096 + (k * 131) % 4000))
            far += model(ln, ln)[0]
            if k % 2:
                toks.append(rnd.randrange(256))
        out.append(_case("one_kind/no_near", toks + T._lits(rnd, 300), far, 0, 0))
        _BUILT["one_kind"] = out
    return _BUILT["one_kind"]


def short():
    """distance D = 1 .. 7: behind the literals a train of (length, D) matches with 0 .. D - 1 literals between them, over several
    chunks.  Whichever token a chunk starts with, a match stands less than D bytes into it: its first D - dw bytes (one to seven)
    come from the output buffer, and the near part behind them repeats them with period D -- the short-period prologue reads
    bytes the far stage has just written.  The tests ask the counters for split pieces in every entry."""
    if "short" not in _BUILT:
        out = []
        for D in range(1, 8):
            rnd = random.Random(50 + D)
            toks, k, pos = T._lits(rnd, PREFIX), 0, PREFIX
            while pos < PREFIX + 12000:
                ln = (3, 9, 20, 33, 258, 8, 31, 5, 12)[k % 9]
                toks.append((ln, D))
                toks += T._lits(rnd, k % D)
                pos += ln + k % D
                k += 1
            out.append(_case("short/D%d" % D, toks + T._lits(rnd, 300), None, None, None))
        _BUILT["short"] = out
    return _BUILT["short"]


# what the commit before the two lists answered for refused()'s stream (status MZHIP_DATA_ERROR, the bytes in front of the
# token, the input up to the verdict, the CRC-32 of those bytes): recorded from its host emulation
REFUSED_PARENT = (-3, 3020, 3178, 1879782367)


def refused():
    """a split piece, ten literals, and a match one byte too far back, all in one chunk"""
    if "refused" not in _BUILT:
        rnd = random.Random(9)
        prefix = T._lits(rnd, PREFIX)
        tail = T._lits(rnd, 300)
        dw = measure_dw(prefix, 10, T._lits(random.Random(1), 10) + tail)
        assert dw >= 1
        mid = T._lits(rnd, 10)
        good = prefix + [(10, dw + 5)] + mid
        bad_at = len(prefix) + 10 + 10
        z = T.encode([("fixed", good + [(4, bad_at + 1)] + tail, True)])
        _BUILT["refused"] = [dict(name="refused/behind_a_split_piece", z=z, data=T.expand([("fixed", good, True)]), cap=bad_at + 4 + 300, dw=dw)]
    return _BUILT["refused"]


def accepted():
    return edges() + all_split() + one_kind() + short()
