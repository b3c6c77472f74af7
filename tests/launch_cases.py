"""One row per batch entry point of include/mzhip.h -- small inputs, the bare ctypes call and a host reference -- for the
launch-contract tests (tests/test_gpu_launch_contract.py: caller streams, launches in flight together, offsets at and above
2^31 and 2^32) and for tests/test_launch_cases.py, which holds the table itself to its own rules on a CPU.

A row gives
    build(seed)  -> (payloads, caps, extra)   8 entries, each a few hundred bytes to 4 KiB, made by the writers the suite
                                              already has (tests/synth.py, zstd_frames.py, bzip2_blocks.py, crypt_ref.py,
                                              the host builds of the encoders); where the entry point has per-entry statuses
                                              other than 0 and a decoy can tell them apart, one entry ends with one
    decoy(seed)  -> payloads                  same lengths, same caps, same extra; expect() differs in EVERY entry
    expect(payloads, caps, extra) -> [entry]  per entry {"words": {result array: value, bytes or None}, "out": the bytes at
                                              the front of its output region or None, "plain": what a read-back of its
                                              output by the library the header names must give, or None}
    call(lib, batch, results, stream)         the ctypes call and nothing else; returns the call's return code
    results(extra) -> (names, words)          the result arrays of the call (gpu_util.guarded_results)

`extra` holds whatever else the call takes: "dev" (arrays that go to the device with the offsets), "prefix" (bytes the caller
puts at the front of each output region before the launch: the history of a resumed DEFLATE stream) and scalars.  A value of
None in "words" is a word the references say nothing about (the counts of an entry that failed); the encoders whose bytes
are not a format property (DEFLATE, LZMA) are judged by read-back ("plain"), the others (bzip2, Zstandard: their GPU tests
hold them to the host build of the same header byte for byte) by both.

The decoy is what a launch that ignored stream order would read: valid streams or plain data of the same sizes at the same
places, so a wrong result is all it can cause.  A real entry that fails and its decoy differ in the status (a truncated
stream and a whole one of the same length; a damaged check field and the right one); mzhip_wzaes_encrypt_batch's one
per-entry status (-102, a strength outside 1..3) depends on `extra` alone, which the decoy shares, so that row has no
failing entry."""
import bz2
import functools
import hashlib
import lzma as pylzma
import zlib

import numpy as np

from tests import bzip2_blocks as bb
from tests import bzip2_enc_cases as bec
from tests import crypt_ref as cr
from tests import synth
from tests import zstd_enc_cases as zec
from tests import zstd_frames as zf
from tests import zstd_large_cases as zlc

N = 8
OUT_FULL, BUF_ERROR, DATA_ERROR = -200, -5, -3
PW = b"test123"
GUARD = 64


def _u32(v):
    return int(v) & 0xFFFFFFFF


def _data(seed, k, size):
    """entry k's plain bytes: a slice of the corpus; every (seed, k) another one"""
    return synth.slices(N, size, 1000 + 2 * seed)[k] if k < N else None


def _noise(seed, k, size):
    return np.random.RandomState(7000 + 16 * seed + k).bytes(size)


def _pair(enc, a, b, k0, span=128):
    """(enc(a[:ka]), enc(b[:kb])) of equal length, ka in [k0, k0 + span), kb wherever b[] compresses to one of those lengths"""
    seen = {}
    for k in range(k0, k0 + span):
        seen.setdefault(len(enc(a[:k])), k)
    lo, hi = min(seen), max(seen)
    k, tried = k0, set()
    for _ in range(600):
        k = min(max(k, 16), len(b))
        while k in tried:
            k += 1
        tried.add(k)
        z = enc(b[:k])
        if len(z) in seen:
            return enc(a[:seen[len(z)]]), z
        k += (lo - len(z)) if len(z) < lo else -((len(z) - hi + 1) // 2) if len(z) > hi else 1
    raise AssertionError("no two streams of one length near %d bytes" % k0)


def _cut_pair(enc, a, b, k0):
    """(a stream of a[] cut to the length of a whole stream of b[:k0], that stream): the entry that fails and its decoy"""
    zb = enc(b[:k0])
    za = enc(a[:3 * k0])
    assert len(za) > len(zb) + 8
    return za[:len(zb)], zb


# ---- the table's machinery ----------------------------------------------------------------------------------------------

class Row:
    kind = "codec"            # "codec": input, output with caps; "sum": one offset array, no output; "crypt": output, no caps
    cap_tied = False          # an encoder whose bound arithmetic the header ties to in_len (no giant out_cap for it)
    names = ("out_len", "in_used", "crc", "status")

    def __init__(self, name):
        self.name = name

    def results(self, extra):
        return self.names, {}

    @functools.lru_cache(maxsize=None)
    def _both(self, seed):
        return self.make(seed)

    def build(self, seed):
        real, _, caps, extra = self._both(seed)
        return list(real), list(caps), extra

    def decoy(self, seed):
        return list(self._both(seed)[1])

    def readback(self, z, i, extra, n):
        """the plain bytes of entry i's output z, by the library the header names (n: the plain length)"""
        raise NotImplementedError


def _decoded(ref, payloads, caps, hist=None):
    """expect() of a decoder: ref(z, i) -> (status, bytes, in_used)"""
    out = []
    for i, z in enumerate(payloads):
        st, data, used = ref(z, i)
        pre = hist[i] if hist else b""
        if st == 0 and len(pre) + len(data) > caps[i]:
            st = OUT_FULL
        if st == 0:
            out.append(dict(words=dict(status=0, out_len=len(pre) + len(data), in_used=used, crc=zlib.crc32(data)), out=pre + data, plain=None))
        else:
            out.append(dict(words=dict(status=_u32(st), out_len=None, in_used=None, crc=None), out=None, plain=None))
    return out


def _io(b):
    return (b["p_in"], b["in_off"].data_ptr(), b["in_len"].data_ptr()), (b["p_out"], b["out_off"].data_ptr(), b["out_cap"].data_ptr())


def _p(t):
    return t.data_ptr() if t is not None else None


def _res(R, *names):
    return [R[k].data_ptr() for k in names]


# ---- raw DEFLATE ---------------------------------------------------------------------------------------------------------

def _deflater(level, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    def enc(d):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        return c.compress(d) + c.flush()
    return enc


def _zlib_ref(z, zdict=None):
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    try:
        out = d.decompress(z)
    except zlib.error:
        return DATA_ERROR, b"", 0
    return (0, out, len(z) - len(d.unused_data)) if d.eof else (BUF_ERROR, out, len(z))


_INFLATE_PLAN = ((1, 400), (6, 900), (9, 2500), ("stored", 1500), (6, 6000), ("huffman", 1500), (6, 3500), ("cut", 1500))


class Inflate(Row):
    def make(self, seed):
        real, dec, caps = [], [], []
        for k, (lv, k0) in enumerate(_INFLATE_PLAN):
            a, b = _data(seed, k, 8192 + 4 * k0), _data(seed + 1000, k, 8192 + 4 * k0)
            if lv == "stored":
                za, zb = synth.stored_blocks(a[:k0], block=1000), synth.stored_blocks(b[:k0], block=1000)
            elif lv == "cut":
                za, zb = _cut_pair(_deflater(6), a, b, k0)
            else:
                za, zb = _pair(_deflater(6, zlib.Z_HUFFMAN_ONLY) if lv == "huffman" else _deflater(lv), a, b, k0)
            st, out, _ = _zlib_ref(za)
            real.append(za)
            dec.append(zb)
            caps.append(len(out) + (k % 3) * 5 if st == 0 else 4096)
        return real, dec, caps, {}

    def expect(self, payloads, caps, extra):
        return _decoded(lambda z, i: _zlib_ref(z), payloads, caps)

    def call(self, L, b, R, stream):
        i, o = _io(b)
        return L.mzhip_inflate_batch(*i, *o, b["n"], *_res(R, "out_len", "in_used", "crc", "status"), stream)


class InflateResume(Row):
    """every entry is taken up at a block header behind history the caller kept (the stream was written with that history as
    its dictionary, so its matches reach into it); entry 0 is a fresh stream without a state's flag; d_stop is asked for"""
    names = ("out_len", "in_used", "crc", "status", "stop")

    def results(self, extra):
        return self.names, {"stop": 4}

    def make(self, seed):
        real, dec, caps, hist, state = [], [], [], [], []
        for k, (lv, k0) in enumerate(_INFLATE_PLAN):
            a, b = _data(seed, k, 8192 + 4 * k0), _data(seed + 1000, k, 8192 + 4 * k0)
            h = b"" if k == 0 else _data(seed + 2000, k, 8192)[:200 + 300 * k]
            lvl = lv if isinstance(lv, int) else 6
            if lv == "cut":
                za, zb = _cut_pair(_deflater(lvl, zdict=h), a, b, k0)
            else:
                za, zb = _pair(_deflater(lvl, zdict=h), a, b, k0)
            st, out, _ = _zlib_ref(za, h)
            real.append(za)
            dec.append(zb)
            hist.append(h)
            caps.append(len(h) + len(out) + (k % 3) * 5 if st == 0 else len(h) + 4096)
            state.append((0, 0, len(h), 1 if k else 0))
        return real, dec, caps, dict(dev=dict(resume=np.array(state, dtype=np.int32)), prefix=hist)

    def expect(self, payloads, caps, extra):
        e = _decoded(lambda z, i: _zlib_ref(z, extra["prefix"][i]), payloads, caps, extra["prefix"])
        for x in e:
            x["words"]["stop"] = None
        return e

    def call(self, L, b, R, stream):
        i, o = _io(b)
        return L.mzhip_inflate_resume_batch(*i, *o, b["n"], *_res(R, "out_len", "in_used", "crc", "status"), _p(b["x"]["resume"]),
                                            _p(R["stop"]), stream)


# ---- checksums and digests -----------------------------------------------------------------------------------------------

_SUM_SIZES = (300, 4096, 257, 1023, 2049, 333, 777, 3000)
_SHA = {20: hashlib.sha1, 22: hashlib.sha224, 23: hashlib.sha256, 24: hashlib.sha384, 25: hashlib.sha512}


class Sum(Row):
    kind = "sum"

    def __init__(self, name, which):
        Row.__init__(self, name)
        self.which = which
        self.names = ({"crc": "crc", "adler": "adler", "sha": "digest"}[which],)

    def results(self, extra):
        return self.names, ({"digest": 16 if extra["alg"] in (24, 25) else 8} if self.which == "sha" else {})

    def make(self, seed):
        real = [(_data(seed, k, 4096) if k & 1 else _noise(seed, k, 4096))[:s] for k, s in enumerate(_SUM_SIZES)]
        dec = [(_data(seed + 1000, k, 4096) if k & 1 else _noise(seed + 1000, k, 4096))[:s] for k, s in enumerate(_SUM_SIZES)]
        extra = {}
        if self.which == "crc":
            extra["dev"] = dict(init=np.random.RandomState(seed).randint(0, 2**32, size=N, dtype=np.uint32).view(np.int32))
        if self.which == "sha":
            extra["alg"] = sorted(_SHA)[seed % 5]
        return real, dec, [0] * N, extra

    def expect(self, payloads, caps, extra):
        out = []
        for i, d in enumerate(payloads):
            if self.which == "crc":
                w = dict(crc=zlib.crc32(d, _u32(extra["dev"]["init"][i])))
            elif self.which == "adler":
                w = dict(adler=zlib.adler32(d))
            else:
                dg = _SHA[extra["alg"]](d).digest()
                w = dict(digest=dg + bytes((64 if extra["alg"] in (24, 25) else 32) - len(dg)))
            out.append(dict(words=w, out=None, plain=None))
        return out

    def call(self, L, b, R, stream):
        i, _ = _io(b)
        if self.which == "crc":
            return L.mzhip_crc32_batch(*i, b["n"], _p(b["x"]["init"]), _p(R["crc"]), stream)
        if self.which == "adler":
            return L.mzhip_adler32_batch(*i, b["n"], _p(R["adler"]), stream)
        return L.mzhip_sha_batch(*i, b["n"], b["extra"]["alg"], _p(R["digest"]), stream)


# ---- LZMA, .xz, bzip2, Zstandard decode ------------------------------------------------------------------------------------

_LZMA_PLAN = (((3, 0, 2), 400, "text"), ((0, 4, 1), 1500, "text"), ((3, 0, 2), 3000, "noise"), ((4, 0, 0), 900, "text"),
              ((1, 2, 2), 6000, "text"), ((0, 0, 2), 2500, "text"), ((3, 0, 2), 9000, "text"), ((3, 0, 2), 1500, "cut"))


def _zip14(lc, lp, pb):
    def enc(d):
        raw = pylzma.compress(d, format=pylzma.FORMAT_ALONE, filters=[dict(id=pylzma.FILTER_LZMA1, preset=6, lc=lc, lp=lp, pb=pb, dict_size=1 << 16)])
        return bytes([5, 2, 5, 0]) + raw[:5] + raw[13:]
    return enc


def _lzma_ref(z):
    """liblzma on a ZIP method-14 payload (the end marker closes it; bytes behind it are not consumed)"""
    d = pylzma.LZMADecompressor(format=pylzma.FORMAT_ALONE)
    try:
        out = d.decompress(z[4:9] + b"\xff" * 8 + z[9:])
    except pylzma.LZMAError:
        return DATA_ERROR, b"", 0
    return (0, out, len(z) - len(d.unused_data)) if d.eof else (BUF_ERROR, out, len(z))


def _xz_ref(z):
    d = pylzma.LZMADecompressor(format=pylzma.FORMAT_XZ)
    try:
        out = d.decompress(z)
    except pylzma.LZMAError:
        return DATA_ERROR, b"", 0
    return (0, out, len(z) - len(d.unused_data)) if d.eof else (BUF_ERROR, out, len(z))


class Lzma(Row):
    """text at lc3 (the slot kernel), noise and lc + lp = 4 (given back to the full-model kernel through the retry list, the
    literal model's upper half in the per-wave scratch); d_max_out = the exact size for every second entry, none for the others"""

    def __init__(self, name, xz):
        Row.__init__(self, name)
        self.xz = xz

    def make(self, seed):
        real, dec, caps = [], [], []
        for k, ((lc, lp, pb), k0, what) in enumerate(_LZMA_PLAN):
            src = _noise if what == "noise" else _data
            a, b = src(seed, k, 8192 + 4 * k0), src(seed + 1000, k, 8192 + 4 * k0)
            if self.xz:
                f = [{"id": pylzma.FILTER_LZMA2, "lc": lc, "lp": lp, "pb": pb, "dict_size": 1 << 16}]
                chk = (pylzma.CHECK_CRC32, pylzma.CHECK_CRC64, pylzma.CHECK_SHA256, pylzma.CHECK_NONE)[k % 4]
                enc = lambda d, f=f, chk=chk: pylzma.compress(d, format=pylzma.FORMAT_XZ, check=chk, filters=f)     # noqa: E731
            else:
                enc = _zip14(lc, lp, pb)
            za, zb = _cut_pair(enc, a, b, k0) if what == "cut" else _pair(enc, a, b, k0)
            st, out, _ = (_xz_ref if self.xz else _lzma_ref)(za)
            real.append(za)
            dec.append(zb)
            caps.append(len(out) + (k % 3) * 5 if st == 0 else 8192)
        max_out = np.array([caps[k] - (k % 3) * 5 if k % 2 == 0 and k != 7 else -1 for k in range(N)], dtype=np.int64)
        return real, dec, caps, dict(dev=dict(max_out=max_out))

    def expect(self, payloads, caps, extra):
        ref = _xz_ref if self.xz else _lzma_ref
        e = _decoded(lambda z, i: ref(z), payloads, caps)
        for i, x in enumerate(e):          # the clamp (PROP_TOTAL_OUT_MAX): length and CRC cover the prefix; the bytes behind it are the entry's own
            mo = int(extra["dev"]["max_out"][i])
            if x["words"]["status"] == 0 and 0 <= mo < x["words"]["out_len"]:
                x["out"] = x["out"][:mo]
                x["words"].update(out_len=mo, crc=zlib.crc32(x["out"]))
                x["clamped"] = True
        return e

    def call(self, L, b, R, stream):
        i, o = _io(b)
        fn = L.mzhip_xz_batch if self.xz else L.mzhip_lzma_batch
        return fn(*i, *o, _p(b["x"]["max_out"]), b["n"], *_res(R, "out_len", "in_used", "crc", "status"), stream)


def _bz_ref(z):
    d = bz2.BZ2Decompressor()
    try:
        out = d.decompress(z)
    except (OSError, ValueError):
        return DATA_ERROR, b"", 0
    return (0, out, len(z) - len(d.unused_data)) if d.eof else (BUF_ERROR, out, len(z))


class Bzip2(Row):
    def make(self, seed):
        real, dec, caps = [], [], []
        plan = ((1, 400, "text"), (9, 900, "text"), (5, 2500, "noise"), (9, 1500, "text"), (1, 4000, "text"), (9, 3000, "run"), (3, 2000, "text"))
        for k, (lv, k0, what) in enumerate(plan):
            src = _noise if what == "noise" else _data
            a, b = src(seed, k, 8192 + 4 * k0), src(seed + 1000, k, 8192 + 4 * k0)
            if what == "run":
                a, b = a[:700] + bytes([a[0]]) * 3000 + a[700:], b[:500] + bytes([b[1]]) * 3000 + b[500:]
            za, zb = _pair(lambda d, lv=lv: bz2.compress(d, lv), a, b, k0)
            real.append(za)
            dec.append(zb)
            caps.append(len(bz2.decompress(za)) + (k % 3) * 5)
        # the failing entry: two blocks, the second with a damaged block CRC (tests/bzip2_blocks.py); its decoy is the whole stream
        T = bb._text(700, seed + 1)
        real.append(bb.write_stream([bb.block(T[:300]), bb.block(T[300:], crc=1)]))
        dec.append(bb.write_stream([bb.block(T[:300]), bb.block(T[300:])]))
        assert len(real[-1]) == len(dec[-1])
        caps.append(4096)
        return real, dec, caps, {}

    def expect(self, payloads, caps, extra):
        return _decoded(lambda z, i: _bz_ref(z), payloads, caps)

    def call(self, L, b, R, stream):
        i, o = _io(b)
        return L.mzhip_bzip2_batch(*i, *o, b["n"], *_res(R, "out_len", "in_used", "crc", "status"), stream)


def _zstd_frames(seed, dk):
    """8 entries of the frame writer of tests/zstd_frames.py: Raw, RLE and Compressed blocks, Huffman literals in one and in four
    streams, sequences, two frames with a skippable one between, checksums -- and one whose checksum is wrong (dk = 0) or
    right (the decoy).  Texts of another seed give streams of the same lengths where no entropy coder is involved; the
    Huffman entries are paired by length."""
    T = [zf.text(2600, 50 * seed + k + 1) for k in range(N)]
    out = []
    f = zf.Frame(single=True, fcs_bytes=2)
    f.content = T[0][:1500]
    out.append(f.raw(T[0][:1500]).bytes())
    out.append(None)                                       # 1: Huffman literals, one stream, checksum (paired below)
    f = zf.Frame()
    out.append(f.comp(T[2][:300], seqs=[(120, 30, 63), (80, 10, 1)]).bytes())
    f = zf.Frame()
    out.append(f.rle(T[3][0], 900).raw(T[3][:700]).bytes())
    f, g = zf.Frame(), zf.Frame(checksum=True)
    g.content = T[4][:400]
    out.append(f.raw(T[4][400:1000]).bytes() + zf.skippable(3, T[4][:21]) + g.raw(T[4][:400]).bytes())
    out.append(None)                                       # 5: Huffman literals, four streams
    f = zf.Frame(checksum=True, checksum_xor=0 if dk else 1)
    f.content = T[6][:800]
    out.append(f.raw(T[6][:300]).raw(T[6][300:800]).bytes())
    f = zf.Frame()
    out.append(f.comp(T[7][:500], seqs=[(200, 40, 103), (100, 8, 2), (50, 300, 203)], lit_mode="raw").bytes())
    return out, T


def _zstd_huf(streams, checksum):
    def enc(d):
        f = zf.Frame(checksum=checksum)
        f.content = d
        return f.comp(d, lit_mode="huf", lit_streams=streams).bytes()
    return enc


def _zstd_ref(z, cap):
    st, data, used = zf.expand(z, cap)
    return st, data, used


class Zstd(Row):
    def make(self, seed):
        real, T = _zstd_frames(seed, 0)
        dec, U = _zstd_frames(seed + 1000, 1)
        real[1], dec[1] = _pair(_zstd_huf(1, True), T[1], U[1], 700, 64)
        real[5], dec[5] = _pair(_zstd_huf(4, False), T[5], U[5], 1600, 64)
        assert [len(z) for z in real] == [len(z) for z in dec]
        caps = []
        for k, z in enumerate(real):
            st, data, _ = zf.expand(z)
            caps.append(len(data) + (k % 3) * 5)
        return real, dec, caps, {}

    def expect(self, payloads, caps, extra):
        # (tests/test_gpu_zstd.py: a failing stream is read with the out_cap it gets; length, bytes and CRC of the complete blocks
        # in front of its problem are compared too, in_used for status 0 alone)
        out = []
        for z, cap in zip(payloads, caps):
            st, data, used = zf.expand(z, cap)
            out.append(dict(words=dict(status=_u32(st), out_len=len(data), in_used=used if st == 0 else None, crc=zlib.crc32(data)),
                            out=data, plain=None))
        return out

    def call(self, L, b, R, stream):
        i, o = _io(b)
        return L.mzhip_zstd_batch(*i, *o, b["n"], *_res(R, "out_len", "in_used", "crc", "status"), stream)


# ---- the crypt streams ---------------------------------------------------------------------------------------------------

_CRYPT_SIZES = (300, 4000, 257, 1023, 2049, 333, 777, 3000)


def _plain(seed, k):
    return (_data(seed, k, 4096) if k & 1 else _noise(seed, k, 4096))[:_CRYPT_SIZES[k]]


class Crypt(Row):
    kind = "crypt"
    names = ("out_len", "status")

    def __init__(self, name, aes, write):
        Row.__init__(self, name)
        self.aes, self.write = aes, write

    def _over(self, k):
        return 4 * (1 + k % 3) + 16 if self.aes else 12

    def make(self, seed):
        verify = [0x10000 | ((17 * k + seed) & 255) << 8 | ((29 * k + 3 * seed) & 255) for k in range(N)]
        strength = [1 + k % 3 for k in range(N)]
        dev = dict(strength=np.array(strength, dtype=np.uint8)) if self.aes else dict(verify=np.array(verify, dtype=np.uint32).view(np.int32))
        seeds = [100 * seed + k + 1 for k in range(N)]
        if self.write:
            real, dec = [_plain(seed, k) for k in range(N)], [_plain(seed + 1000, k) for k in range(N)]
            if self.aes:
                rec = b"".join(bytes(np.random.RandomState(s).randint(0, 256, size=4 * st + 4, dtype=np.uint8)) + bytes([0xEE] * (12 - 4 * st))
                               for s, st in zip(seeds, strength))
                dev["salt"] = np.frombuffer(rec, dtype=np.uint8).copy()
            else:
                dev["header"] = np.frombuffer(b"".join(bytes(np.random.RandomState(s).randint(0, 256, size=10, dtype=np.uint8)) for s in seeds),
                                              dtype=np.uint8).copy()
            caps = [len(d) + self._over(k) for k, d in enumerate(real)]
            return real, dec, caps, dict(dev=dev, seeds=seeds)
        real, dec = [], []
        for k in range(N):
            for dst, sd in ((real, seed), (dec, seed + 1000)):
                d = _plain(sd, k)
                if self.aes:
                    z = cr.wz_encrypt(PW, d, strength[k], salt_seed=seeds[k] + (sd - seed))
                    if k == 7 and dst is real:      # the authentication code differs: -105, and the bytes ARE delivered
                        z = z[:-1] + bytes([z[-1] ^ 1])
                else:
                    ok = not (k == 7 and dst is real)       # the check byte differs: -108, nothing is written
                    z = cr.pk_encrypt(PW, d, (verify[k] >> 8) & 255, (verify[k] & 255) ^ (0 if ok else 0x40), header_seed=seeds[k] + (sd - seed))
                dst.append(z)
        caps = [len(z) - self._over(k) for k, z in enumerate(real)]
        return real, dec, caps, dict(dev=dev, seeds=seeds)

    def expect(self, payloads, caps, extra):
        out = []
        for k, p in enumerate(payloads):
            if self.write:
                v = int(extra["dev"]["verify"].view(np.uint32)[k]) if not self.aes else 0
                z = cr.wz_encrypt(PW, p, int(extra["dev"]["strength"][k]), salt_seed=extra["seeds"][k]) if self.aes else \
                    cr.pk_encrypt(PW, p, (v >> 8) & 255, v & 255, header_seed=extra["seeds"][k])
                st = 0
            elif self.aes:
                st, z = cr.wz_decrypt(PW, p, int(extra["dev"]["strength"][k]))
            else:
                st, z = cr.pk_decrypt(PW, p, int(extra["dev"]["verify"].view(np.uint32)[k]))
            out.append(dict(words=dict(status=_u32(st), out_len=len(z)), out=z, plain=None, exact_region=True))
        return out

    def call(self, L, b, R, stream):
        i, o = _io(b)
        x, n = b["x"], b["n"]
        r = _res(R, "out_len", "status")
        if self.write and self.aes:
            return L.mzhip_wzaes_encrypt_batch(*i, _p(x["strength"]), _p(x["salt"]), o[0], o[1], n, PW, len(PW), *r, stream)
        if self.write:
            return L.mzhip_pkcrypt_encrypt_batch(*i, o[0], o[1], n, PW, len(PW), _p(x["verify"]), _p(x["header"]), *r, stream)
        if self.aes:
            return L.mzhip_wzaes_batch(*i, _p(x["strength"]), o[0], o[1], n, PW, len(PW), *r, stream)
        return L.mzhip_pkcrypt_batch(*i, o[0], o[1], n, PW, len(PW), _p(x["verify"]), *r, stream)


# ---- the encoders --------------------------------------------------------------------------------------------------------

_ENC_SIZES = (300, 4096, 257, 1023, 2049, 333, 3333, 3000)


def _enc_inputs(seed):
    """text, a run, noise (entry 7: into a quarter of its size, OUT_FULL; its decoy is a run, which fits)"""
    real, dec = [], []
    for k, s in enumerate(_ENC_SIZES):
        a, b = _data(seed, k, 4096)[:s], _data(seed + 1000, k, 4096)[:s]
        if k == 3:
            a, b = a[:100] + bytes([a[5]]) * (s - 200) + a[100:200], b[:50] + bytes([b[6]]) * (s - 200) + b[50:200]
        if k in (4, 7):
            a = _noise(seed, k, s)
            b = _noise(seed + 1000, k, s) if k == 4 else bytes([b[0]]) * s
        real.append(a)
        dec.append(b)
    return real, dec


class Encoder(Row):
    names = ("out_len", "crc", "status")

    def results(self, extra):
        return self.names, {}

    def _judged(self, payloads, caps, extra, small_ok):
        """expect() of an encoder judged by read-back: status 0 and the input's CRC where the header's bound is met, OUT_FULL for
        noise into a quarter of its size; an entry of neither kind does not belong in the table"""
        out = []
        for i, d in enumerate(payloads):
            if caps[i] >= small_ok(len(d)):
                out.append(dict(words=dict(status=0, out_len=None, crc=zlib.crc32(d)), out=None, plain=d))
            elif len(set(d)) == 1 and len(d) >= 1024:      # (a run of one value: a few dozen bytes in every format here)
                out.append(dict(words=dict(status=0, out_len=None, crc=zlib.crc32(d)), out=None, plain=d))
            else:
                assert len(zlib.compress(d, 9)) > caps[i] + 64, "an entry whose status the header does not settle"
                out.append(dict(words=dict(status=_u32(OUT_FULL), out_len=None, crc=None), out=None, plain=None))
        return out


class Deflate(Encoder):
    def __init__(self, name, leveled):
        Row.__init__(self, name)
        self.leveled = leveled

    def make(self, seed):
        real, dec = _enc_inputs(seed)
        caps = [len(d) + len(d) // 8 + 64 for d in real]
        caps[7] = len(real[7]) // 4
        extra = dict(dev=dict(final=np.array([1 - (k % 3 == 1) for k in range(N)], dtype=np.uint8)))
        if self.leveled:
            extra["level"], extra["window"] = ((6, 15), (9, 12), (1, 9), (4, 15))[seed % 4]
        return real, dec, caps, extra

    def expect(self, payloads, caps, extra):
        return self._judged(payloads, caps, extra, lambda k: k + k // 8 + 64)

    def readback(self, z, i, extra, n):
        d = zlib.decompressobj(-extra.get("window", 15))
        out = d.decompress(z)
        assert d.eof == bool(extra["dev"]["final"][i]) and not d.unused_data, ("final", i)
        return out

    def call(self, L, b, R, stream):
        i, o = _io(b)
        r = _res(R, "out_len", "crc", "status")
        if self.leveled:
            return L.mzhip_deflate_batch_level(*i, *o, _p(b["x"]["final"]), b["n"], b["extra"]["level"], b["extra"]["window"], *r, stream)
        return L.mzhip_deflate_batch(*i, *o, _p(b["x"]["final"]), b["n"], *r, stream)


class LzmaEncode(Encoder):
    def __init__(self, name, preset):
        Row.__init__(self, name)
        self.preset = preset

    def make(self, seed):
        real, dec = _enc_inputs(seed)
        caps = [len(d) + len(d) // 8 + 1024 for d in real]
        caps[7] = len(real[7]) // 4
        # mode 1 (the payload of one LZMA2 chunk) for compressible entries of at least one byte
        extra = dict(dev=dict(mode=np.array([1 if k in (1, 5, 6) else 0 for k in range(N)], dtype=np.uint8)), max_in=max(len(d) for d in real))
        if self.preset:
            extra["preset"] = (6, 1, 9)[seed % 3]
        return real, dec, caps, extra

    def expect(self, payloads, caps, extra):
        return self._judged(payloads, caps, extra, lambda k: k + k // 8 + 1024)

    def readback(self, z, i, extra, n):
        if not extra["dev"]["mode"][i]:
            return pylzma.decompress(z[4:9] + b"\xff" * 8 + z[9:], format=pylzma.FORMAT_ALONE)
        body = bytes([0xE0 | ((n - 1) >> 16), ((n - 1) >> 8) & 255, (n - 1) & 255, (len(z) - 1) >> 8, (len(z) - 1) & 255, 0x5D]) + z + b"\x00"
        return pylzma.decompress(body, format=pylzma.FORMAT_RAW, filters=[{"id": pylzma.FILTER_LZMA2, "dict_size": 8 << 20}])

    def call(self, L, b, R, stream):
        i, o = _io(b)
        r = _res(R, "out_len", "crc", "status")
        if self.preset:
            return L.mzhip_lzma_encode_batch_preset(*i, b["extra"]["max_in"], *o, _p(b["x"]["mode"]), b["n"], b["extra"]["preset"], *r, stream)
        return L.mzhip_lzma_encode_batch(*i, b["extra"]["max_in"], *o, _p(b["x"]["mode"]), b["n"], *r, stream)


class EmulEncoder(Encoder):
    """bzip2 and Zstandard: every word and every byte from the host build of the same header (tests/emul), one emulated wave
    per expect() in list order, and libbz2 / the frame reader of tests/zstd_frames.py read the bytes back"""
    cap_tied = True

    def __init__(self, name, zstd):
        Row.__init__(self, name)
        self.zstd = zstd

    def make(self, seed):
        real, dec = _enc_inputs(seed)
        if self.zstd:
            level, flags = ((3, 1), (1, 0), (9, 1), (19, 0))[seed % 4]
            extra = dict(level=level, flags=flags, max_in=max(len(d) for d in real))
            caps = [14 + len(d) + 3 for d in real]                        # mzhip_zstd_encode_bound for at most one block
        else:
            level = (9, 1, 5, -1)[seed % 4]
            extra = dict(level=level, max_in=max(len(d) for d in real))
            caps = [int(bec.load_emul().emul_bzip2_enc_bound(len(d), level)) for d in real]
        caps[7] = len(real[7]) // 4
        return real, dec, caps, extra

    def expect(self, payloads, caps, extra):
        out = []
        if self.zstd:
            E = zec.load_emul()
            w = E.emul_zstd_enc_wave_new()
        else:
            E = bec.load_emul()
            w = E.emul_bzip2_enc_wave_new(extra["max_in"])
        for d, cap in zip(payloads, caps):
            st, z, crc = zec.emul_encode(w, d, extra["level"], extra["flags"], cap) if self.zstd else bec.emul_encode(w, d, extra["level"], cap)
            if st == 0:
                out.append(dict(words=dict(status=0, out_len=len(z), crc=zlib.crc32(d)), out=z, plain=d))
                assert crc == zlib.crc32(d)
            else:
                out.append(dict(words=dict(status=_u32(st), out_len=0, crc=None), out=None, plain=None))
        (E.emul_zstd_enc_wave_free if self.zstd else E.emul_bzip2_enc_wave_free)(w)
        return out

    def readback(self, z, i, extra, n):
        if self.zstd:
            st, data, used = zf.expand(z)
            assert (st, used) == (0, len(z)), ("frame", i, st)
            return data
        return bz2.decompress(z)

    def call(self, L, b, R, stream):
        i, o = _io(b)
        r = _res(R, "out_len", "crc", "status")
        x = b["extra"]
        if self.zstd:
            return L.mzhip_zstd_encode_batch(*i, x["max_in"], *o, b["n"], x["level"], x["flags"], *r, stream)
        return L.mzhip_bzip2_encode_batch(*i, x["max_in"], *o, b["n"], x["level"], *r, stream)


ROWS = [
    Inflate("mzhip_inflate_batch"), InflateResume("mzhip_inflate_resume_batch"),
    Sum("mzhip_crc32_batch", "crc"), Sum("mzhip_adler32_batch", "adler"),
    Lzma("mzhip_lzma_batch", False), Lzma("mzhip_xz_batch", True), Bzip2("mzhip_bzip2_batch"), Zstd("mzhip_zstd_batch"),
    Sum("mzhip_sha_batch", "sha"),
    Crypt("mzhip_pkcrypt_batch", False, False), Crypt("mzhip_wzaes_batch", True, False),
    Crypt("mzhip_pkcrypt_encrypt_batch", False, True), Crypt("mzhip_wzaes_encrypt_batch", True, True),
    Deflate("mzhip_deflate_batch", False), Deflate("mzhip_deflate_batch_level", True),
    LzmaEncode("mzhip_lzma_encode_batch", False), LzmaEncode("mzhip_lzma_encode_batch_preset", True),
    EmulEncoder("mzhip_bzip2_encode_batch", False), EmulEncoder("mzhip_zstd_encode_batch", True),
]
BY_NAME = {r.name: r for r in ROWS}
NO_FAILING_ENTRY = {"mzhip_crc32_batch", "mzhip_adler32_batch", "mzhip_sha_batch",        # no per-entry status at all
                    "mzhip_pkcrypt_encrypt_batch",                                          # always 0
                    "mzhip_wzaes_encrypt_batch"}                                            # -102 depends on d_strength alone (see above)


def differs(a, b):
    """do two entries of expect() differ in a result word both name, in the bytes or in what a read-back gives?"""
    for k, v in a["words"].items():
        w = b["words"].get(k)
        if v is not None and w is not None and v != w:
            return True
    return (a["out"] is not None and b["out"] is not None and a["out"] != b["out"]) or \
           (a["plain"] is not None and b["plain"] is not None and a["plain"] != b["plain"])


def verify(row, exp, extra, words, region, where):
    """a launch against expect(): words = {result array: uint32 [n] or [n, w]} as the device left them, region(i) = the bytes
    of entry i's output region.  Every word the reference names, the bytes at the front of the region, the read-back."""
    for i, e in enumerate(exp):
        for k, want in e["words"].items():
            if want is None:
                continue
            got = words[k][i]
            if isinstance(want, bytes):
                assert got.tobytes() == want, (where, row.name, i, k)
            else:
                assert int(got) == _u32(want), (where, row.name, i, k, int(got), _u32(want))
        if e["out"] is not None:
            assert region(i)[:len(e["out"])] == e["out"], (where, row.name, i, "bytes")
        if e["plain"] is not None:
            ol = int(words["out_len"][i])
            r = region(i)
            assert ol <= len(r), (where, row.name, i, ol)
            assert row.readback(r[:ol], i, extra, len(e["plain"])) == e["plain"], (where, row.name, i, "read-back")


# ---- the two synchronous, device-resident calls --------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def _expand(z, cap):
    """zf.expand of a large entry, once per process: the frame reader is plain Python, seconds per MiB"""
    return zf.expand(z, cap)


class Large:
    """one entry of about 300 KiB compressed; the decoy is a shorter stream of other data brought to the same length by what
    the format allows behind a stream (bytes DEFLATE does not consume; a skippable Zstandard frame)"""

    def __init__(self, name, zstd):
        self.name, self.zstd = name, zstd

    @functools.lru_cache(maxsize=8)
    def _both(self, seed):
        c = synth.corpus()
        k = (37 * seed) % 1000
        if not self.zstd:
            a = (c[k:] + c * 2)[:1 << 20]
            b = (c[::-1][k:] + c)[:900000]
            za, zb = synth.deflate_raw(a, 6), synth.deflate_raw(b, 6)
            assert 250000 < len(zb) < len(za) < 400000
            return za, zb + bytes(len(za) - len(zb)), len(a) + 5
        progs = [p for p in zlc.cases() if p[2] == 0 and not zlc.over_cap(p[0])]

        def stream(d, level, rot):
            E = zec.load_emul()
            w = E.emul_zstd_enc_wave_new()
            st, z, _ = zec.emul_encode(w, d, level, 1)
            E.emul_zstd_enc_wave_free(w)
            assert st == 0
            ps = [p for p in progs if len(p[1]) <= 3500]                           # the same programs, in another order
            ps = ps[rot % len(ps):] + ps[:rot % len(ps)]
            return b"".join(p[1] for p in ps[:len(ps) * 2 // 3]) + z + b"".join(p[1] for p in ps[len(ps) * 2 // 3:])
        a = synth.markov_entries(1, (1 << 20) + 1, seed=11 + seed)[0]        # (the encoder's matches reach 8 MiB back: no tiling)
        b = synth.markov_entries(1, 800000, seed=511 + seed)[0]
        za, zb = stream(a, 3, seed), stream(b, 3, seed + 4)
        assert 150000 < len(zb) + 8 <= len(za) < 500000, (len(za), len(zb))
        zb += zf.skippable(5, bytes(len(za) - len(zb) - 8))
        return za, zb, len(_expand(za, 1 << 30)[1]) + 5

    def build(self, seed):
        za, _, cap = self._both(seed)
        return za, cap

    def decoy(self, seed):
        return self._both(seed)[1]

    def expect(self, z, cap):
        if self.zstd:
            st, data, used = _expand(z, 1 << 30)
            st, data, used = (st, data, used) if len(data) <= cap else _expand(z, cap)
        else:
            st, data, used = _zlib_ref(z)
        assert st == 0 and len(data) <= cap
        return dict(words=dict(status=0, out_len=len(data), in_used=used, crc=zlib.crc32(data)), out=data, plain=None)

    def call(self, L, p_in, in_len, p_out, cap, res, stream):
        """res: four ctypes words (out_len, in_used, crc, status)"""
        import ctypes as C

        r = [C.byref(x) for x in res]
        if self.zstd:
            return L.mzhip_zstd_large(p_in, in_len, p_out, cap, 0, *r, None, stream)
        return L.mzhip_inflate_large(p_in, in_len, p_out, cap, *r, stream)


LARGE = [Large("mzhip_inflate_large", False), Large("mzhip_zstd_large", True)]
