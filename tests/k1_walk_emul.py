"""The host emulation of K1 alone (tests/emul/k1_walk_main.cpp over minizip-ng_amd/csrc/inflate_core.h), shared by
tests/test_walk_refill_emul.py and tests/test_chase_lean_emul.py: the two libraries both judge -- the product's span limit and
record caps, and caps and spans so low that every window runs into them -- and the sanitised stand-alone program."""
import ctypes as C
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "k1_walk_main.cpp")
_u8p = C.POINTER(C.c_uint8)
CAPS = ["-DMZ_CHASE_SMAX=512u", "-DMZ_REC_CAP1=16u", "-DMZ_REC_CAP2=8u"]
BUILDS = [("product", []), ("product_caps", CAPS)]
_LIBS = {}


def build_variant(tag, flags):
    """the library of one build, compiled once per process and tag"""
    if tag not in _LIBS:
        out = os.path.join(ROOT, "tests", "emul", "_build")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "libemul_k1_walk_%s.so" % tag)
        subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL"] + flags +
                       ["-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"), "-shared", "-fPIC", SRC, "-o", so], check=True)   # (K1 alone: emul.cpp holds every core)
        L = C.CDLL(so)
        L.emul_inflate.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32] + [C.POINTER(C.c_uint32)] * 3
        _LIBS[tag] = (L, list(flags))
    assert _LIBS[tag][1] == list(flags), tag
    return _LIBS[tag][0]


def builds():
    """{tag: library}: the product at its span limit and record caps, and at 512 bits / 16 / 8 steps"""
    with ThreadPoolExecutor(max_workers=2) as ex:
        libs = list(ex.map(lambda b: build_variant(*b), BUILDS))
    return {tag: lib for (tag, _), lib in zip(BUILDS, libs)}


def run_sanitised(tmp_path, sweep, streams_and_caps):
    """k1_walk_main.cpp under AddressSanitizer and UBSan over [(stream, capacity)], sweep "in" or "out" -> its lines as tuples
    (case, misalignment, status, out_len, in_used, crc); a report of the sanitizer fails the caller with the report"""
    exe = str(tmp_path / "k1_walk_main")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"), SRC, "-o", exe], check=True)
    blob = struct.pack("<I", len(streams_and_caps)) + b"".join(struct.pack("<II", len(z), cap) + z for z, cap in streams_and_caps)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    p = subprocess.run([exe, sweep, str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == 16 * len(streams_and_caps)
    return [tuple(int(x) for x in line.split()) for line in lines]
