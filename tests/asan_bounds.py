#!/usr/bin/env python3
"""Child process of tests/test_kernel_emul.py::test_emul_bounds_under_asan (not collected by pytest): replays the case list of
tests/test_gpu_bounds.py through a -fsanitize=address,undefined build of the 64-lane host emulation.  Input and output of every
call are heap allocations of EXACTLY in_len and out_cap bytes made with the process's malloc -- AddressSanitizer's, preloaded
into this child only -- so the allocation itself is the red zone, for reads as well as writes (the one place where an
over-READ of a core can be seen: the device has no such check).
    LD_PRELOAD=$(gcc -print-file-name=libasan.so) ASAN_OPTIONS=detect_leaks=0 python tests/asan_bounds.py <libemul_asan.so>"""
import ctypes as C
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import synth  # noqa: E402
from tests import test_gpu_bounds as cases  # noqa: E402

libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p
libc.malloc.argtypes = [C.c_size_t]
libc.free.argtypes = [C.c_void_p]
u32p = C.POINTER(C.c_uint32)
# include/mzhip.h: a core reads its input in aligned 32-bit words, so the bytes of the aligned words that hold the first and the
# last byte of an entry's input must be readable (at most 3 in front, 3 behind); the block starts 0 .. 3 bytes in front of the data on a word boundary and ends on the next one
IN_DWORD = 4


class Heap:
    """a malloc()ed block of exactly n bytes (n == 0: a block of 0 bytes -- nothing of it may be touched)"""

    def __init__(self, n, data=None, pad_to=1, mis=0):
        """mis: the block starts that many bytes in front of the data (an input that is not word-aligned)"""
        self.n = n
        self.base = libc.malloc((mis + n + pad_to - 1) // pad_to * pad_to)
        assert self.base or n == 0
        self.p = (self.base or 0) + mis
        if data:
            C.memmove(self.p, data, n)

    def bytes(self, k):
        return C.string_at(self.p, k)

    def free(self):
        libc.free(self.base)


def main(so):
    L = C.CDLL(so)
    dec = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    for name in ("emul_inflate", "emul_inflate_steps"):
        getattr(L, name).argtypes = dec + [u32p] * 3
    for name in ("emul_lzma", "emul_lzma_slots", "emul_xz"):
        getattr(L, name).argtypes = dec + [C.c_int64] + [u32p] * 3
    for name in ("emul_deflate", "emul_deflate_lazy", "emul_deflate_best"):
        getattr(L, name).argtypes = dec + [C.c_uint32] + [u32p] * 2
    L.emul_lzma_encode_ways.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, u32p, u32p]
    calls = 0

    def decode(fn, z, cap, *extra):
        nonlocal calls
        calls += 1
        a, o = Heap(len(z), z, IN_DWORD, calls % 4), Heap(cap)
        ol, iu, crc = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = fn(a.p, len(z), o.p, cap, *extra, C.byref(ol), C.byref(iu), C.byref(crc))
        assert ol.value <= cap
        out = o.bytes(ol.value)
        assert a.bytes(len(z)) == z
        a.free()
        o.free()
        return st, out, crc.value

    def encode(fn, d, cap, pre=(), post=()):
        nonlocal calls
        calls += 1
        a, o = Heap(len(d), d, IN_DWORD, calls % 4), Heap(cap)
        ol, crc = C.c_uint32(), C.c_uint32()
        st = fn(a.p, len(d), *pre, o.p, cap, *post, C.byref(ol), C.byref(crc))
        assert ol.value <= cap or st != 0
        out = o.bytes(ol.value) if st == 0 else b""
        assert a.bytes(len(d)) == d
        a.free()
        o.free()
        return st, out, crc.value

    # raw DEFLATE: both front ends, exact cap, cap - 1, half, 0
    for name, z, d in cases.inflate_cases():
        if name.startswith("slice") and name not in ("slice0", "slice1", "slice40", "slice41"):
            continue
        for fn in (L.emul_inflate, L.emul_inflate_steps):
            assert decode(fn, z, len(d)) == (0, d, zlib.crc32(d)), name
            for cap in {max(len(d) - 1, 0), len(d) // 2, 0}:
                st = decode(fn, z, cap)[0]
                assert st == (0 if cap >= len(d) else -200), (name, cap, st)
    far0 = cases.fixed_stream([(258, 1), 65, 66])
    far100 = cases.fixed_stream(list(synth.corpus()[:100]) + [(258, 32768), 67])
    for z in (far0, far100):
        for fn in (L.emul_inflate, L.emul_inflate_steps):
            assert decode(fn, z, 8192)[0] == -3
    for name, _, z in synth.edge_payloads()[:8]:
        for cname, bad in synth.corruptions(z):
            decode(L.emul_inflate, bad, 70000)
    # LZMA (full model and slot build) and XZ: exact cap with and without the size, cap - 1, the clamp
    for name, z, d in cases.lzma_cases():
        for fn in (L.emul_lzma, L.emul_lzma_slots):
            for mo in (len(d), -1):
                st, out, crc = decode(fn, z, len(d), C.c_int64(mo))
                assert st == -300 and fn is L.emul_lzma_slots or (st, out, crc) == (0, d, zlib.crc32(d)), (name, st)
            if d:
                st = decode(fn, z, len(d) - 1, C.c_int64(-1))[0]
                assert st in (-200, -300), (name, st)
            k = len(d) * 2 // 3
            st, out, crc = decode(fn, z, len(d), C.c_int64(k))
            assert st == -300 or (st, out, crc) == (0, d[:k], zlib.crc32(d[:k])), (name, st)
    for i, (name, d, x) in enumerate(synth.xz_cases()):
        if len(d) > 120000 or (i % 3 and len(d) > 2000):
            continue
        assert decode(L.emul_xz, x, len(d), C.c_int64(-1)) == (0, d, zlib.crc32(d)), name
        if d:
            assert decode(L.emul_xz, x, len(d) - 1, C.c_int64(-1))[0] == -200, name
        k = len(d) * 2 // 3
        assert decode(L.emul_xz, x, len(d), C.c_int64(k)) == (0, d[:k], zlib.crc32(d[:k])), name
    # the encoders: the documented cap, cap == len and len // 4 on incompressible bytes, final and non-final pieces
    text, noise = cases._enc_inputs()
    for fn in (L.emul_deflate, L.emul_deflate_lazy, L.emul_deflate_best):
        for w in (15, 9):
            L.emul_deflate_window(w)
            for i, d in enumerate(text + noise):
                final = 1 - (i % 3 == 1)
                st, z, crc = encode(fn, d, len(d) + len(d) // 8 + 64, post=(final,))
                dec = zlib.decompressobj(-w)
                assert st == 0 and dec.decompress(z) == d and dec.eof == bool(final) and crc == zlib.crc32(d), (w, i)
            for d in noise:
                for cap in (len(d), len(d) // 4):
                    assert encode(fn, d, cap, post=(1,))[0] == -200, (w, len(d), cap)
        L.emul_deflate_window(15)
    for ways in (1, 4):
        for i, d in enumerate(text + noise):
            mode = 1 if (i % 2 and 0 < len(d) <= 65536 and i < len(text)) else 0
            st, z, crc = encode(L.emul_lzma_encode_ways, d, len(d) + len(d) // 8 + 1024, pre=(mode, ways))
            assert st == 0 and cases._unwrap_lzma(z, mode, len(d)) == d and crc == zlib.crc32(d), (ways, i)
        for d in noise:
            for cap in (len(d), len(d) // 4):
                assert encode(L.emul_lzma_encode_ways, d, cap, pre=(0, ways))[0] == -200, (ways, len(d), cap)
    print("asan bounds replay ok: %d calls" % calls)


if __name__ == "__main__":
    main(sys.argv[1])
