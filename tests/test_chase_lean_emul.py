"""CPU tests of two build knobs of K1 in the 64-lane host emulation of the shipped sources: MZ_CHASE_LEAN (inflate_walk.inc: a chase
takes its next target in front of a trip, a step only ever stops a chase) and MZ_NEAR_PACKED (inflate_commit.inc: the near
batches' rank searches on byte offsets with a scalar first step, the short-period prologue from a packed constant).  Every knob
at 0 and at 1, alone and together, at the product's span limit and record caps and once more with caps and spans so low that
every window runs into them.  The cases are those of tests/chase_lean_cases.py; zlib is the judge of status, bytes, consumed
input and CRC, and the settings agree with each other byte for byte.

The last test compiles tests/emul/chase_lean_main.cpp, a program of its own, with -fsanitize=address,undefined and runs it as
a child process over the same cases."""
import ctypes as C
import os
import struct
import subprocess
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import chase_lean_cases as CL
from tests.test_kernel_emul import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = C.POINTER(C.c_uint8)
CAPS = ["-DMZ_CHASE_SMAX=512u", "-DMZ_REC_CAP1=16u", "-DMZ_REC_CAP2=8u"]
BUILDS = [("a%db%d%s" % (a, b, "_caps" if caps else ""), ["-DMZ_CHASE_LEAN=%d" % a, "-DMZ_NEAR_PACKED=%d" % b] + (CAPS if caps else []))
          for caps in (False, True) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))]


def _build_variant(tag, flags):
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libemul_lean_%s.so" % tag)
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL"] + flags +
                   ["-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"), "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "emul", "chase_lean_main.cpp"), "-o", so], check=True)   # (K1 alone)
    L = C.CDLL(so)
    L.emul_inflate.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
    return L


@pytest.fixture(scope="module")
def builds():
    """{tag: library} of every knob setting at the product's span limit and record caps, and at 512 bits / 16 / 8 steps"""
    with ThreadPoolExecutor(max_workers=4) as ex:
        libs = list(ex.map(lambda b: _build_variant(*b), BUILDS))
    return {tag: lib for (tag, _), lib in zip(BUILDS, libs)}


def test_cases_are_zlibs():
    """the expected bytes of every case are what zlib makes of its stream, and zlib sees its end at the stream's last byte"""
    names = set()
    for name, z, data, cap in CL.everything():
        d = zlib.decompressobj(-15)
        assert d.decompress(z) == data and d.eof and d.unused_data == b"", name
        assert cap >= len(data)
        names.add(name)
    assert len(names) == len(CL.everything())
    assert {"retarget/flat8-cap2", "retarget/short-codes-cap1", "near/D3/lits0", "near/D7/run"} <= names


def _check(tag, L, case, mis, omis):
    name, z, data, cap = case
    st, iu, out, crc = _run(L.emul_inflate, z, cap, mis=mis, omis=omis)
    assert st == 0, (tag, name, mis, omis, st)
    if out != data:
        bad = next((k for k in range(min(len(out), len(data))) if out[k] != data[k]), min(len(out), len(data)))
        raise AssertionError("%s: %s (mis %d, omis %d): byte %d of %d differs (got %d bytes)" % (tag, name, mis, omis, bad, len(data), len(out)))
    assert iu == len(z) and crc == zlib.crc32(data), (tag, name, mis, omis, iu, len(z))


def test_retarget_cases(builds):
    """every retarget case through every build: small spans, long steps, block ends and both record caps"""
    t0 = time.time()
    cases = [c for c in CL.everything() if c[0].startswith("retarget/")]
    assert len(cases) == 57
    for tag, L in builds.items():
        for k, case in enumerate(cases):
            _check(tag, L, case, (k * 5) % 16, (k * 3 + 1) % 16)
    print("test_retarget_cases: %d builds x %d cases, %.1f s" % (len(builds), len(cases), time.time() - t0))


def test_near_cases_every_staging_phase(builds):
    """every near case with the output pointer at the misalignments that put the chunk's first byte at staging index 0, 1, 15
    (and the piece behind 0 / 1 / 15 / 16 fresh literals at 0 .. 31) -- the staging index of a byte is its offset in the chunk
    plus the 16-byte misalignment of where the chunk lands"""
    t0 = time.time()
    cases = [c for c in CL.everything() if c[0].startswith(("near/", "tails/"))]
    assert len(cases) == 77
    for tag, L in builds.items():
        for k, case in enumerate(cases):
            for omis in ((0, 1, 15) if not tag.endswith("_caps") else ((k * 7) % 16,)):
                _check(tag, L, case, (k * 3) % 16, omis)
    print("test_near_cases_every_staging_phase: %d builds x %d cases, %.1f s" % (len(builds), len(cases), time.time() - t0))


def test_knobs_change_no_result(builds):
    """status, bytes, consumed input and CRC of every case are those of the build with both knobs off (the code before them)"""
    base = builds["a0b0"]
    for k, (name, z, data, cap) in enumerate(CL.everything()):
        want = _run(base.emul_inflate, z, cap, mis=5, omis=(k * 11) % 16)
        for tag, L in builds.items():
            if not tag.endswith("_caps"):
                assert _run(L.emul_inflate, z, cap, mis=5, omis=(k * 11) % 16) == want, (tag, name)


def test_sanitised_program(tmp_path):
    """tests/emul/chase_lean_main.cpp under AddressSanitizer and UBSan, the default (product) knobs: every case at sixteen output
    misalignments from heap blocks that end with the input's last aligned dword and the output's capacity.  Its verdicts are
    zlib's."""
    t0 = time.time()
    exe = str(tmp_path / "chase_lean_main")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"),
                    os.path.join(ROOT, "tests", "emul", "chase_lean_main.cpp"), "-o", exe], check=True)
    cases = [c for c in CL.everything() if len(c[2]) <= 40000]        # (the sanitised emulation is slow: the long runs once, below)
    cases += [c for c in CL.everything() if len(c[2]) > 40000][:2]
    blob = struct.pack("<I", len(cases)) + b"".join(struct.pack("<II", len(c[1]), c[3]) + c[1] for c in cases)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == 16 * len(cases)
    for line in lines:
        c, omis, st, ol, iu, crc = (int(x) for x in line.split())
        name, z, data, _ = cases[c]
        assert (st, ol, iu, crc) == (0, len(data), len(z), zlib.crc32(data)), (name, omis, st, ol, iu)
    print("test_sanitised_program: %d cases x 16 misalignments, %.1f s" % (len(cases), time.time() - t0))
