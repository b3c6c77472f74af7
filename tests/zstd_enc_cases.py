"""The inputs of the Zstandard encoder tests (tests/test_zstd_enc_emul.py on the host build, tests/test_gpu_zstd_enc.py on the
device): the smallest shapes at which each stage of minizip-ng_amd/csrc/zstd_enc_core.h can go wrong.  cases() ->
[(name, data, level, flags)], computed once; small() = the ones of at most 700 bytes; big() = the one entry that takes the
window-descriptor path (8 MiB + 70 000 bytes), kept apart because it alone takes seconds.  Inputs whose structure matters
are PLANTED: noise (no 4 bytes of it repeat) for literals, copies of earlier noise for matches, so the parse has one choice.
load_emul() builds and binds the host build of the header (tests/emul/emul_zstd_enc.cpp); emul_streams() = what it writes for
every case, the bytes the device must write too."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import synth

FAR_DICT = 8 << 20      # MZ_LZE_FAR_DICT: up to here a frame is Single_Segment
BLOCK = 65536


class Plan:
    """bytes made of noise and copies: lit(n) appends n fresh noise bytes, copy(d, n) n bytes from d back (d < n overlaps, as a
    match does).  A copy ends where it is told to: the byte behind it differs from the one the match would go on with."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.b = bytearray()
        self.stop = None     # the byte the next literal must not be

    def lit(self, n):
        for _ in range(n):
            v = int(self.rs.randint(0, 256))
            while v == self.stop:
                v = int(self.rs.randint(0, 256))
            self.b.append(v)
            self.stop = None
        return self

    def copy(self, d, n):
        assert 0 < d <= len(self.b)
        if self.stop is not None:      # a copy right behind a copy: it must not go on the first one
            assert self.b[len(self.b) - d] != self.stop, "pick another distance"
        for _ in range(n):
            self.b.append(self.b[len(self.b) - d])
        self.stop = self.b[len(self.b) - d]
        return self

    def fill_to(self, n):
        return self.lit(n - len(self.b))

    def bytes(self):
        return bytes(self.b)


def noise(n, seed):
    return np.random.RandomState(seed).bytes(n)


def unique_noise(n, seed):
    """noise in which no 4 bytes repeat (the first seed from `seed` on that gives it): not even a chance match"""
    while True:
        b = np.frombuffer(noise(n, seed), dtype=np.uint8).astype(np.uint32)
        grams = b[:-3] | (b[1:-2] << 8) | (b[2:-1] << 16) | (b[3:] << 24)
        if np.unique(grams).size == grams.size:
            return b.astype(np.uint8).tobytes()
        seed += 1000


def de_bruijn(k, n):
    """the de Bruijn sequence B(k, n) over 0 .. k - 1: every n-gram once, so no n bytes of it repeat"""
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(seq)


def skewed(n, lo, count, seed):
    """n bytes over the values lo .. lo + count - 1 with geometric-like frequencies: Huffman pays, 4-grams rarely repeat"""
    rs = np.random.RandomState(seed)
    w = 1.0 / (np.arange(count) + 4.0)
    return (rs.choice(count, size=n, p=w / w.sum()) + lo).astype(np.uint8).tobytes()


_CASES = None
_BIG = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    T = synth.corpus()
    Cs = []

    def add(name, data, level=3, flags=0):
        Cs.append((name, bytes(data), level, flags))

    # ---- lengths: prose, and noise in front of one match (Raw literals of exactly k bytes: their size formats)
    for k in (0, 1, 2, 3, 4, 5, 63, 64, 65, 16383, 16384, 65535, 65536, 65537, 131073):
        add("len_%d" % k, T[1000:1000 + k], 3, k & 1)
    for k in (31, 32, 4095, 4096):
        add("raw_literals_%d" % k, Plan(k).lit(k).copy(k, min(k, 200)).bytes())
    # ---- literal content
    add("one_value_70000", b"\xfb" * 70000)                                   # RLE blocks
    add("one_value_literals", Plan(1).lit(300).bytes() + b"z" * 40 + Plan(1).lit(300).bytes() * 2)
    p = Plan(2).lit(BLOCK)                                                       # second block: "kkk", 300 bytes of the first, "kk"
    p.b += b"kkk"
    p.copy(BLOCK, 300)
    add("rle_literals", p.bytes() + b"kk")
    add("two_values", bytes(np.random.RandomState(5).randint(0, 2, 3000).astype(np.uint8) * 7 + 48))
    add("uniform_256", b"".join(np.random.RandomState(6).permutation(256).astype(np.uint8).tobytes() for _ in range(12)))
    db8 = de_bruijn(8, 4)                                                        # 4096 bytes over 8 values, no match possible
    for k in (1023, 1024):
        add("streams_%d" % k, bytes(v + 97 for v in db8[:k]))                  # one or four Huffman streams; nseq = 0
    add("no_match_4096", bytes(v * 9 + 3 for v in db8))
    add("low_values", db8[:700])                                                 # values 0 .. 7: a direct description is 5 bytes
    for count in (128, 129, 130):
        add("symbols_%d" % count, skewed(6000, 0, count, 20 + count))
    add("bytes_high", skewed(5000, 128, 128, 31))
    add("bytes_all", skewed(9000, 0, 256, 32))
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    skew = np.repeat(np.arange(20, dtype=np.uint8) * 11 + 5, fib)
    np.random.RandomState(7).shuffle(skew)
    add("fibonacci_frequencies", skew.tobytes())
    # ---- sequence counts, literal lengths, match lengths
    for nseq in (127, 128):
        p = Plan(40 + nseq).lit(1200)
        for i in range(nseq):
            p.lit(3).copy(len(p.b) - 9 * i, 8)
        add("nseq_%d" % nseq, p.lit(3).bytes())
    p = Plan(50).lit(400).copy(350, 9)
    for ll in (15, 16, 17, 1, 0):
        p.lit(ll).copy(len(p.b) - 13 * ll - 3, 9)
    add("literal_lengths", p.bytes())
    p = Plan(51)
    p.b += unique_noise(65000, 51)
    add("literal_run_65000", p.copy(30000, 200).bytes())
    p = Plan(52).lit(2000)
    for k, ml in enumerate((34, 35, 36, 273, 274, 277, 546, 600)):
        p.lit(2).copy(len(p.b) - 40 * k, ml)
    add("match_lengths", p.lit(1).bytes())
    add("match_run_60000", Plan(53).lit(100).copy(100, 60000).lit(50).bytes())
    for d in (1, 2, 3):
        add("distance_%d" % d, Plan(54 + d).lit(50).copy(d, 500).lit(20).copy(d + 20, 30).bytes())
    # ---- repeat offsets
    A, B, Cd = 301, 417, 533
    p = Plan(60).lit(700)
    p.copy(A, 8).lit(2).copy(A, 8)                                   # rep0, literals between
    p.lit(2).copy(B, 8).lit(2).copy(A, 8)                            # rep1
    p.lit(2).copy(B, 8).lit(2).copy(Cd, 8).lit(2).copy(A, 8)         # rep2
    add("rep_with_literals", p.lit(3).bytes())
    p = Plan(61).lit(700)
    p.lit(2).copy(A, 8).copy(B, 8).copy(A, 8)                        # ll == 0: value 1 names rep1
    p.lit(2).copy(Cd, 8).lit(2).copy(B, 8).copy(A + 40, 8).copy(Cd, 8)   # ll == 0: value 2 names rep2
    p.lit(2).copy(A, 8).copy(A - 1, 8)                               # ll == 0: value 3 names rep0 - 1
    add("rep_without_literals", p.lit(3).bytes())
    p = Plan(62).lit(700)
    for i in range(40):
        p.lit(1 + i % 3).copy(A if i & 1 else B, 7)
    add("rep_alternating", p.lit(2).bytes())
    head = Plan(63).lit(20000).copy(20000, 20000)
    head.fill_to(BLOCK - 24).copy(500, 8).lit(8).copy(700, 8)
    assert len(head.b) == BLOCK
    seam = Plan(64)
    seam.b, seam.stop = bytearray(head.b), head.stop
    add("rep_across_seam", seam.lit(5).copy(500, 8).lit(30).copy(700, 9).lit(4).bytes())
    raw = Plan(65)
    raw.b, raw.stop = bytearray(head.b), head.stop
    add("rep_across_raw_block", raw.lit(BLOCK).lit(5).copy(700, 8).lit(30).copy(500, 9).lit(4).bytes())
    # ---- reach
    add("reach_32768", Plan(66).lit(32768).copy(32768, 100).lit(10).bytes())
    add("reach_100k_twice", noise(100 * 1024, 67) * 2, 3, 1)
    # ---- incompressible: every block Raw
    for k in (1000, 65536, 65538, 200000):
        add("noise_%d" % k, noise(k, 70 + k % 7), 3, k == 65538)
    # ---- the corpus, and the levels
    add("corpus_64k", T[:BLOCK], 3, 1)
    add("corpus_1m", synth.markov_entries(1, 1 << 20, seed=9)[0], 3, 0)
    for level in (1, 3, 9, 19, -1):
        add("levels_%d" % level, T[70000:70000 + 150000], level)
    _CASES = Cs
    return Cs


def small():
    return [c for c in cases() if len(c[1]) <= 700]


def big():
    """the window-descriptor path: one entry of 8 MiB + 70 000 bytes of generated text"""
    global _BIG
    if _BIG is None:
        _BIG = ("markov_8m_70000", synth.markov_entries(1, FAR_DICT + 70000, seed=11)[0], 1, 1)
    return _BIG


# ---- the host build -------------------------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minizip-ng_amd", "csrc")
EMUL_SRC = os.path.join(ROOT, "tests", "emul", "emul_zstd_enc.cpp")
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)


def build_emul(name="libemul_zstd_enc.so", src=EMUL_SRC, extra=()):
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    subprocess.run(["g++", "-O2", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + CSRC, "-shared", "-fPIC", src, "-o", so] + list(extra),
                   check=True)
    return so


_EMUL = None


def load_emul():
    global _EMUL
    if _EMUL is None:
        L = C.CDLL(build_emul())
        L.emul_zstd_enc_wave_new.restype = C.c_void_p
        L.emul_zstd_enc_wave_free.argtypes = [C.c_void_p]
        L.emul_zstd_enc_run.restype = C.c_int32
        L.emul_zstd_enc_run.argtypes = [C.c_void_p, _u8p, C.c_uint32, _u8p, C.c_uint32, C.c_int32, C.c_uint32, _u32p, _u32p]
        L.emul_zstd_enc_lds_bytes.restype = C.c_uint32
        L.emul_zstd_enc_scratch_bytes.restype = C.c_uint32
        L.emul_zstd_enc_bound.restype = C.c_uint64
        L.emul_zstd_enc_bound.argtypes = [C.c_uint32]
        L.emul_zstd_enc_max_nseq.restype = C.c_uint32
        L.emul_zstd_enc_max_nseq.argtypes = [C.c_int]
        _EMUL = L
    return _EMUL


def emul_encode(wave, data, level, flags=0, cap=None):
    """-> (status, frame, crc) of one entry through an emulated wave, in plain buffers"""
    L = load_emul()
    cap = int(L.emul_zstd_enc_bound(len(data))) if cap is None else cap
    src = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = (C.c_uint8 * max(cap, 1))()
    ol, crc = C.c_uint32(0), C.c_uint32(0)
    st = L.emul_zstd_enc_run(wave, src, len(data), out, cap, level, flags, C.byref(ol), C.byref(crc))
    return st, bytes(out[:ol.value]), crc.value


_STREAMS = None


def emul_streams():
    """{name: frame} of every case, through one emulated wave in list order"""
    global _STREAMS
    if _STREAMS is None:
        L = load_emul()
        w = L.emul_zstd_enc_wave_new()
        _STREAMS = {}
        for name, data, level, flags in cases():
            st, z, _ = emul_encode(w, data, level, flags)
            assert st == 0, name
            _STREAMS[name] = z
        L.emul_zstd_enc_wave_free(w)
    return _STREAMS
