"""CPU tests of K1's commit stage on the 64-lane host emulation (tests/emul/emul.cpp built with -DMZHIP_HOST_EMUL), once per
setting of MZ_CRC_CHAINS in {1, 2, 4} (the CRC fold of C super-tiles of a lane together, crc32_core.h).  The entries are
tests/commit_chain_cases.py's -- the group boundaries of the fold, and the tails of near copies (inflate_core.h mz_copy32_seq)
behind the groups of records the emit rounds load (inflate_emit.inc); zlib judges bytes and CRC, and every build must give the
same four result words for every entry."""
import ctypes as C
import os
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import commit_chain_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = C.POINTER(C.c_uint8)
KNOBS = [1, 2, 4]


def _build(c):
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libemul_commit_c%d.so" % c)
    subprocess.run(["g++", "-O1", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DMZ_CRC_CHAINS=%d" % c,
                    "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"), "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "emul", "emul.cpp"), "-o", so], check=True)
    return so


@pytest.fixture(scope="module")
def builds():
    """{chains: library}"""
    with ThreadPoolExecutor(4) as ex:
        sos = list(ex.map(_build, KNOBS))
    libs = {}
    for k, so in zip(KNOBS, sos):
        L = C.CDLL(so)
        L.emul_inflate.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
        L.emul_inflate.restype = C.c_int32
        libs[k] = L
    return libs


def _run(L, z, cap):
    """-> (status, out_len, in_used, crc), the bytes; the output buffer is poisoned and 64 bytes longer than cap"""
    src = (C.c_uint8 * (len(z) + 16)).from_buffer_copy(z + bytes(16))
    out = (C.c_uint8 * (cap + 64)).from_buffer_copy(b"\xA5" * (cap + 64))
    ol, iu, crc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    st = L.emul_inflate(src, len(z), out, cap, C.byref(ol), C.byref(iu), C.byref(crc))
    raw = bytes(out)
    assert raw[cap:] == b"\xA5" * 64
    return (st, ol.value, iu.value, crc.value), raw[:cap]


def _check(builds, entries):
    for name, z, data in entries:
        d = zlib.decompressobj(-15)
        assert d.decompress(z) == data and d.eof and not d.unused_data, name      # (the judge, of the case itself)
        want = (0, len(data), len(z), zlib.crc32(data))
        for i, cap in enumerate((len(data), len(data) + 37)):
            first = None
            for knobs in KNOBS if i == 0 else KNOBS[-1:]:
                words, got = _run(builds[knobs], z, cap)
                assert words == want, (name, knobs, cap, words, want)
                assert got[:len(data)] == data, (name, knobs, cap)
                first = first or words
                assert words == first, (name, knobs)                              # the builds agree on every result word


def test_crc_group_boundaries(builds):
    """(a) output sizes on, before and behind every group boundary of the CRC fold, four stream forms each"""
    es = cases.sizes()
    assert len(es) == 4 * len(cases.SIZES) and {len(d) for _, _, d in es} == set(cases.SIZES)
    _check(builds, es)


def test_near_copy_tails(builds):
    """(b) every match length 3 .. 40, 255 .. 258 at every distance of 1 .. 9, 15 .. 17, 31 .. 33: near, behind 6 KiB of
    literals, and in a train that crosses chunk starts"""
    es = cases.tails()
    assert len(es) == 3 * len(cases.DISTANCES)
    for d in cases.DISTANCES:
        for what in ("near", "far"):
            prog_bytes = next(e for e in es if e[0] == "tails/D%d/%s" % (d, what))
            assert len(prog_bytes[2]) >= sum(cases.LENGTHS)                       # every length is in it once
    _check(builds, es)
