"""The inputs of the bzip2 encoder tests (tests/test_bzip2_enc_emul.py on the host build, tests/test_gpu_bzip2_enc.py on the
device): the smallest shapes at which each stage of minizip-ng_amd/csrc/bzip2_enc_core.h can go wrong.  cases() ->
[(name, data, level)], computed once; small() = the ones of at most 700 bytes.  load_emul() builds and binds the host build of the
header (tests/emul/emul_bzip2_enc.cpp); emul_streams() = what it writes for every case, the bytes the device must write too."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import bzip2_blocks as bb
from tests import bzip2_tokens as bt

BMAX1 = 100000 - 19   # symbols a level-1 block holds behind the first run-length stage


def no_runs(n, seed):
    """n bytes of noise in which no two neighbours are equal: the first run-length stage leaves them as they are"""
    rs = np.random.RandomState(seed)
    step = rs.randint(1, 256, size=n).astype(np.int64)
    return (np.cumsum(step) % 256).astype(np.uint8).tobytes()


def prose(n, seed):
    """generated prose: words of a small vocabulary, spaces, now and then a full stop and a line end"""
    import random
    rnd = random.Random(seed)
    words = [bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(1, 10))) for _ in range(600)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
        out += b" " if rnd.random() < 0.9 else b".\n"
    return bytes(out[:n])


def fibonacci_word(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def with_symbol_count(target, seed):
    """noise over 64 byte values whose one block codes exactly `target` symbols (end of block included)"""
    src = (np.random.RandomState(seed).randint(0, 64, size=target + 400) + 48).astype(np.uint8).tobytes()
    n = target - 1
    for _ in range(200):
        got = bt.n_symbols(src[:n])
        if got == target:
            return src[:n]
        n += target - got
    raise AssertionError("no input with %d symbols" % target)


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    rs = np.random.RandomState(12)
    T = bb._text(70000, seed=3)
    C = []

    def add(name, data, level=9):
        C.append((name, bytes(data), level))

    for k in (0, 1, 2, 3, 4, 5, 63, 64, 65):
        add("len_%d" % k, T[:k])
    for k in (4, 5, 255, 256, 258, 259, 260, 263, 264, 518, 519):
        add("run_%d" % k, b"r" * k)
        add("run_%d_between" % k, b"xy" + b"r" * k + b"zw" + T[:9])
    for k in range(0, 7):   # a run of 600 that starts k symbols in front of the level-1 capacity
        add("run_at_cut_%d" % k, no_runs(BMAX1 - k, 20 + k) + b"\x07" * 600 + T[:100], 1)
    add("one_value", b"\xfb" * (255 * 40))   # runs of 255: four bytes and the count 251, the byte itself -- one value in the block
    add("one_value_3", b"q" * 3)
    add("all_values_once", bytes(range(256)))
    add("all_values_x40", b"".join(rs.permutation(256).astype(np.uint8).tobytes() for _ in range(40)))
    for per in (b"ab", b"abc"):
        for n in (63, 64, 65, 66, 999, 1000, 1001, 1002):
            add("periodic_%s_%d" % (per.decode(), n), (per * 600)[:n])
    add("repeat_3000_x20", rs.bytes(3000) * 20)
    add("fibonacci_50000", fibonacci_word(50000))
    add("zeros_70000", b"\0" * 70000)
    for target in (150, 151, 199, 200, 599, 600, 1199, 1200, 2399, 2400):
        add("symbols_%d" % target, with_symbol_count(target, 40 + target))
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    skew = np.repeat(np.arange(24, dtype=np.uint8) + 65, fib)
    rs.shuffle(skew)
    add("fibonacci_frequencies", skew.tobytes())
    for delta in (-1, 0, 1):
        add("noise_capacity_%+d" % delta, no_runs(BMAX1 + delta, 60), 1)
    long_text = bb._text(BMAX1 + 600, seed=5)
    for delta in (-1, 0, 1):
        add("text_capacity_%+d" % delta, _prefix_with_rle1(long_text, BMAX1 + delta), 1)
    add("three_blocks", bb._prose(250000, 6), 1)
    lv = bb._prose(150000, 8)
    for level in (1, 2, 9, -1):
        add("levels_%d" % level, lv, level)
    _CASES = C
    return C


def _prefix_with_rle1(src, target):
    """a prefix of src that the first run-length stage turns into exactly `target` symbols (its last byte ends no run of 4)"""
    k = len(src)
    n = len(bb.rle1(src))
    while n > target:
        k -= max((n - target) * 4 // 5, 1)
        n = len(bb.rle1(src[:k]))
    while n < target:
        k += 1
        n = len(bb.rle1(src[:k]))
    if n != target:
        raise AssertionError("no prefix with %d symbols" % target)
    return src[:k]


def small():
    return [c for c in cases() if len(c[1]) <= 700]


# ---- the host build -------------------------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minizip-ng_amd", "csrc")
EMUL_SRC = os.path.join(ROOT, "tests", "emul", "emul_bzip2_enc.cpp")
MAX_IN = 250000   # the largest entry of the "launch" an emulated wave belongs to
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)


def build_emul(name="libemul_bzip2_enc.so", src=EMUL_SRC):
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, name)
    subprocess.run(["g++", "-O2", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + CSRC, "-shared", "-fPIC", src, "-o", so],
                   check=True)
    return so


_EMUL = None


def load_emul():
    global _EMUL
    if _EMUL is None:
        L = C.CDLL(build_emul())
        L.emul_bzip2_enc_wave_new.restype = C.c_void_p
        L.emul_bzip2_enc_wave_new.argtypes = [C.c_uint32]
        L.emul_bzip2_enc_wave_free.argtypes = [C.c_void_p]
        L.emul_bzip2_enc_run.restype = C.c_int32
        L.emul_bzip2_enc_run.argtypes = [C.c_void_p, _u8p, C.c_uint32, _u8p, C.c_uint32, C.c_int32, _u32p, _u32p]
        L.emul_bzip2_enc_lds_bytes.restype = C.c_uint32
        L.emul_bzip2_enc_scratch_bytes.restype = C.c_uint64
        L.emul_bzip2_enc_scratch_bytes.argtypes = [C.c_uint32, C.c_int32]
        L.emul_bzip2_enc_bound.restype = C.c_uint64
        L.emul_bzip2_enc_bound.argtypes = [C.c_uint32, C.c_int32]
        _EMUL = L
    return _EMUL


def emul_encode(wave, data, level, cap=None):
    """-> (status, stream, crc) of one entry through an emulated wave, in plain buffers"""
    L = load_emul()
    cap = int(L.emul_bzip2_enc_bound(len(data), level)) if cap is None else cap
    src = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = (C.c_uint8 * max(cap, 1))()
    ol, crc = C.c_uint32(0), C.c_uint32(0)
    st = L.emul_bzip2_enc_run(wave, src, len(data), out, cap, level, C.byref(ol), C.byref(crc))
    return st, bytes(out[:ol.value]), crc.value


_STREAMS = None


def emul_streams():
    """{name: stream} of every case, through one emulated wave in list order"""
    global _STREAMS
    if _STREAMS is None:
        L = load_emul()
        w = L.emul_bzip2_enc_wave_new(MAX_IN)
        _STREAMS = {}
        for name, data, level in cases():
            st, z, _ = emul_encode(w, data, level)
            assert st == 0, name
            _STREAMS[name] = z
        L.emul_bzip2_enc_wave_free(w)
    return _STREAMS
