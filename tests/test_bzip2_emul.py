"""CPU tests of minizip-ng_amd/csrc/bzip2_core.h through its host build (tests/emul/emul_bzip2.cpp, g++ -DMZHIP_HOST_EMUL):
every program family of tests/bzip2_blocks.py and bz2.compress output at the sizes where the format takes another path,
judged by libbz2 (Python's bz2): status, out_len, in_used, bytes and CRC-32 exact.  Entries sit inside patterned buffers
with red zones at several misalignments, and run one after the other through ONE wave's LDS and scratch.  The product
path is the HIP build of the same header (tests/test_gpu_bzip2.py)."""
import ctypes as C
import os
import subprocess
import zipfile
import zlib

import numpy as np
import pytest

from tests import bzip2_blocks as bb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minizip-ng_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emul", "emul_bzip2.cpp")
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
RED = 256


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libemul_bzip2.so")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + CSRC, "-shared", "-fPIC", SRC, "-o", so],
                   check=True)
    L = C.CDLL(so)
    L.emul_bzip2_wave_new.restype = C.c_void_p
    L.emul_bzip2_wave_free.argtypes = [C.c_void_p]
    L.emul_bzip2_run.restype = C.c_int32
    L.emul_bzip2_run.argtypes = [C.c_void_p, _u8p, C.c_uint32, _u8p, C.c_uint32, _u32p, _u32p, _u32p]
    return L


@pytest.fixture()
def wave(emu):
    w = emu.emul_bzip2_wave_new()
    yield w
    emu.emul_bzip2_wave_free(w)


def _pattern(n, seed):
    return np.random.RandomState(seed).randint(1, 256, size=n, dtype=np.uint8)


def run(emu, wave, z, cap, mis=0, omis=0):
    """one entry inside patterned buffers with red zones, at the byte misalignments mis / omis (relative to 16): the input
    is unchanged afterwards, nothing outside [out, out + cap) is written, and with status 0 nothing behind out_len.
    -> (status, out_len, in_used, bytes, crc)"""
    a = _pattern(RED + 16 + len(z) + RED, 211)
    i0 = RED + (-(a.ctypes.data + RED) % 16) + mis
    a[i0:i0 + len(z)] = np.frombuffer(z, dtype=np.uint8)
    a0 = a.copy()
    out = _pattern(RED + 16 + cap + RED, 212)
    o0 = RED + (-(out.ctypes.data + RED) % 16) + omis
    out0 = out.copy()
    ol, iu, crc = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_uint32(0x12345678)
    st = emu.emul_bzip2_run(wave, C.cast(a.ctypes.data + i0, _u8p), len(z), C.cast(out.ctypes.data + o0, _u8p), cap,
                            C.byref(ol), C.byref(iu), C.byref(crc))
    assert (a == a0).all(), "input changed"
    assert ol.value <= cap and iu.value <= len(z)
    keep = np.ones(out.size, dtype=bool)
    keep[o0:o0 + (ol.value if st == 0 else cap)] = False
    bad = np.flatnonzero((out != out0) & keep)
    assert bad.size == 0, "byte at offset %d of the output (status %d, out_len %d, cap %d) was written" % (int(bad[0]) - o0, st, ol.value, cap)
    got = out[o0:o0 + ol.value].tobytes()
    assert crc.value == zlib.crc32(got)
    return st, ol.value, iu.value, got, crc.value


def expect(emu, wave, name, z, st, data, used, cap=None, mis=0, omis=0):
    """the judge's verdict (st, data, used) against the core's"""
    got = run(emu, wave, z, (len(data) if st == 0 else 4096) if cap is None else cap, mis, omis)
    assert got[0] == st, (name, got[0], st)
    if st == 0:
        assert got[1] == len(data) and got[3] == data and got[2] == used and got[4] == zlib.crc32(data), name


def test_layout_fits_the_launch(emu):
    emu.emul_bzip2_lds_bytes.restype = C.c_uint32
    emu.emul_bzip2_scratch_bytes.restype = C.c_uint32
    assert emu.emul_bzip2_lds_bytes() + 1024 <= 160 * 1024 // 8      # 8 single-wave workgroups per CU, each with the CRC byte table
    assert emu.emul_bzip2_scratch_bytes() >= 4 * 900000 + 900000 + 18002 and emu.emul_bzip2_scratch_bytes() % 256 == 0


def test_every_program_one_wave(emu, wave):
    """all families, one behind the other through one wave's state, out_cap exactly the length for the valid ones"""
    for name, z, st, data, used in bb.verdicts():
        expect(emu, wave, name, z, st, data, used, cap=None if st == 0 else 200000)
    for name, z, st, data, used in reversed(bb.verdicts()):
        expect(emu, wave, name, z, st, data, used, cap=(len(data) + 37) if st == 0 else 200000)


@pytest.mark.parametrize("mis,omis", [(0, 0), (1, 3), (2, 1), (3, 2), (7, 15), (13, 5)])
def test_programs_misaligned(emu, wave, mis, omis):
    for name, z, st, data, used in bb.verdicts()[::3]:
        expect(emu, wave, name, z, st, data, used, cap=None if st == 0 else 3000, mis=mis, omis=omis)


def test_compressor_output(emu, wave):
    for k, (name, z, d) in enumerate(bb.payloads()):
        expect(emu, wave, name, z, 0, d, len(z), mis=k % 5, omis=(3 * k) % 7)
        expect(emu, wave, name + "+tail", z + b"\x31\x41tail", 0, d, len(z), mis=(k + 1) % 4)


def test_full_block_then_small_entries(emu, wave):
    """a 900 000-symbol block fills the scratch; what runs behind it on the same wave must not see any of it"""
    z, d = bb.full_block()
    expect(emu, wave, "full", z, 0, d, len(z), mis=1, omis=1)
    for name, z1, st, data, used in bb.verdicts()[:40]:
        expect(emu, wave, name, z1, st, data, used, cap=None if st == 0 else 200000)
    for name, z1, d1 in bb.payloads()[:12]:
        expect(emu, wave, name, z1, 0, d1, len(z1))
    assert run(emu, wave, z, len(d) - 1)[0] == bb.OUT_FULL


def test_out_cap(emu, wave):
    """out_cap equal to the length decodes; one byte less is -200, for a plain byte, a run and a second block alike"""
    T = bb._text(700)
    cases = [bb.write_stream([bb.block(T)]), bb.write_stream([bb.block(T[:300]), bb.block(T[300:])]),
             bb.write_stream([bb.block(b"x" + b"q" * 259)]), bb.write_stream([bb.block(b"q" * 4)]), bb.write_stream([bb.block(b"z")])]
    cases += [z for name, z, d in bb.payloads() if name in ("equal_259_l9", "three_blocks_l1", "equal_1_l1")]
    for z in cases:
        st, data, used = bb.judge(z)
        assert st == 0
        expect(emu, wave, "exact", z, 0, data, used, cap=len(data))
        got = run(emu, wave, z, len(data) - 1, omis=1)
        assert got[0] == bb.OUT_FULL and data.startswith(got[3])
        assert run(emu, wave, z, 0)[0] == bb.OUT_FULL
    assert run(emu, wave, bb.write_stream([]), 0)[:3] == (0, 0, 14)
    # the first problem in stream order decides: a block that does not fit comes before the broken block behind it
    z = bb.write_stream([bb.block(T[:300]), bb.block(T[300:], crc=1)])
    assert run(emu, wave, z, 299)[0] == bb.OUT_FULL and run(emu, wave, z, 700)[0] == bb.DATA_ERROR
    assert run(emu, wave, z, 700)[1] == 300


def test_no_input(emu, wave):
    assert run(emu, wave, b"", 16)[:3] == (bb.BUF_ERROR, 0, 0)
    for k in range(1, 14):
        assert run(emu, wave, bb.write_stream([])[:k], 16)[0] == bb.BUF_ERROR


def _kinds():
    _, z3, d3 = bb.payloads()[-1]
    kinds = [("three_blocks", z3, 0, d3, len(z3))]
    pick = ("all_bytes", "six_groups", "block_crc", "run_at_capacity", "lengths_20", "selectors_18002", "one_byte",
            "four_at_end_no_count", "map_all", "no_end_of_block", "unassigned_code")
    kinds += [v for v in bb.verdicts() if v[0] in pick]
    kinds.append([v for v in bb.verdicts() if v[0].startswith("cut_") and v[2] == bb.BUF_ERROR][12])
    return kinds


def test_each_kind_behind_each_other_kind(emu, wave):
    """what an entry leaves in LDS and scratch -- tables of six groups, 18 002 selectors, a 258-symbol alphabet, links of a longer
    block, an error half-way -- must not reach the next entry"""
    kinds = _kinds()
    assert len(kinds) >= 12
    for a in kinds:
        for b in kinds:
            if a is kinds[0] and b is kinds[0]:
                continue
            expect(emu, wave, a[0], *a[1:], cap=None if a[2] == 0 else 200000)
            expect(emu, wave, a[0] + " -> " + b[0], *b[1:], cap=None if b[2] == 0 else 200000)


def test_reference_seed_archive(emu, wave):
    """the method-12 entry of the reference's fuzzer seed archive, where that tree is at hand"""
    path = "/root/reference/test/fuzz/unzip_fuzzer_seed_corpus/bzip2.zip"
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    raw = open(path, "rb").read()
    with zipfile.ZipFile(path) as zf:
        zi = zf.getinfo("vangogh.gif")
        want = zf.read(zi)
    assert zi.compress_type == 12 and (zi.compress_size, zi.file_size) == (163785, 163825)
    h = zi.header_offset
    p = h + 30 + int.from_bytes(raw[h + 26:h + 28], "little") + int.from_bytes(raw[h + 28:h + 30], "little")
    z = raw[p:p + zi.compress_size]
    expect(emu, wave, "vangogh.gif", z, 0, want, len(z), mis=p % 16)
    assert zlib.crc32(want) == zi.CRC


def test_sanitised_standalone_program(tmp_path):
    """the same core from a program of its own under -fsanitize=address,undefined: a handful of the writer's programs dumped to
    files, exact-size heap buffers, one wave for all of them"""
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "emul_bzip2_san")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DEMUL_BZIP2_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe], check=True)
    pick = ("plain", "all_bytes", "six_groups", "selectors_18002", "lengths_oversubscribed", "unassigned_code", "unassigned_code_short",
            "run_70000", "run_weights_22", "symbols_over_capacity", "no_end_of_block", "four_at_end_no_count", "count_255",
            "block_crc", "map_all", "periodic", "length_21", "selector_value_6", "orig_ptr_cap", "randomised")
    chosen = [v for v in bb.verdicts() if v[0] in pick]
    chosen += [v for v in bb.verdicts() if v[0].startswith("cut_") and v[2] == bb.BUF_ERROR][5:25:5]
    chosen += [(name, z, 0, d, len(z)) for name, z, d in bb.payloads() if name in ("three_blocks_l1", "equal_259_l9", "empty_l1")]
    assert len(chosen) >= 20
    args, want = [], []
    for k, (name, z, st, data, used) in enumerate(chosen):
        f = tmp_path / ("%02d.bz2" % k)
        f.write_bytes(z)
        for cap in ((len(data), max(len(data) - 1, 0)) if st == 0 else (70001,)):
            args += [str(f), str(cap)]
            want.append((name, cap, st, data, used))
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    for (name, cap, st, data, used), line in zip(want, lines):
        got = [int(x) for x in line.split()]
        if st == 0 and cap == len(data):
            assert got == [0, len(data), used, zlib.crc32(data)], name
        elif st == 0:
            assert got[0] == (bb.OUT_FULL if data else 0), name
        else:
            assert got[0] == st, (name, got, st)
