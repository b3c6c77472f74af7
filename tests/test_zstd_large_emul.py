"""CPU tests of the wave-per-block Zstandard reader (minizip-ng_amd/csrc/zstd_par_core.h behind csrc/zstd_parallel.inc) through its
host build (tests/emul/emul_zstd_large.cpp, g++ -DMZHIP_HOST_EMUL): the multi-block programs of tests/zstd_large_cases.py, every
program and payload of tests/zstd_frames.py and libzstd's multi-block output where it loads, at the default window and at
windows of 4096 bytes.  Status, out_len, in_used, bytes and CRC-32 must be the one-wave reader's (the host build of
mz_zstd_entry in the same library) and expand()'s; the counters say whether the blocks were decoded by waves of their own.
The blocks of a pass run in a shuffled order.  The product path is the HIP build of the same text (tests/test_gpu_zstd_large.py)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import zstd_frames as zf
from tests import zstd_large_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minizip-ng_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emul", "emul_zstd_large.cpp")
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
RED = 256
BIG = 400000   # an out_cap that no failing program fills
WINDOWS = (0, 4096)


def build_emul():
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libemul_zstd_large.so")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + CSRC, "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = C.CDLL(so)
    L.emul_zstd_one.restype = C.c_int32
    L.emul_zstd_one.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32, _u32p, _u32p, _u32p]
    L.emul_zstd_large.restype = C.c_int32
    L.emul_zstd_large.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p, _u32p]
    return L


@pytest.fixture(scope="module")
def emu():
    return build_emul()


def _pattern(n, seed):
    return np.random.RandomState(seed).randint(1, 256, size=n, dtype=np.uint8)


def run(emu, z, cap, window=0, mis=0, omis=0, seed=1, one=False):
    """one entry inside patterned buffers with red zones, at the byte misalignments mis / omis (relative to 16): the input is
    unchanged afterwards, nothing outside [out, out + cap) is written, and with status 0 nothing behind out_len.
    -> (status, out_len, in_used, bytes, crc), stats {windows, blocks, borrowed, rounds, fallback}"""
    a = _pattern(RED + 16 + len(z) + RED, 211)
    i0 = RED + (-(a.ctypes.data + RED) % 16) + mis
    a[i0:i0 + len(z)] = np.frombuffer(z, dtype=np.uint8)
    a0 = a.copy()
    out = _pattern(RED + 16 + cap + RED, 212)
    o0 = RED + (-(out.ctypes.data + RED) % 16) + omis
    out0 = out.copy()
    ol, iu, crc = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_uint32(0x12345678)
    stats = (C.c_uint32 * 6)()
    pin, pout = C.cast(a.ctypes.data + i0, _u8p), C.cast(out.ctypes.data + o0, _u8p)
    if one:
        st = emu.emul_zstd_one(pin, len(z), pout, cap, C.byref(ol), C.byref(iu), C.byref(crc))
    else:
        st = emu.emul_zstd_large(pin, len(z), pout, cap, window, seed, C.byref(ol), C.byref(iu), C.byref(crc), stats)
    assert (a == a0).all(), "input changed"
    assert ol.value <= cap and iu.value <= len(z)
    keep = np.ones(out.size, dtype=bool)
    keep[o0:o0 + (ol.value if st == 0 else cap)] = False
    bad = np.flatnonzero((out != out0) & keep)
    assert bad.size == 0, "byte at offset %d of the output (status %d, out_len %d, cap %d) was written" % (int(bad[0]) - o0, st, ol.value, cap)
    got = out[o0:o0 + ol.value].tobytes()
    assert crc.value == zlib.crc32(got)
    return (st, ol.value, iu.value, got, crc.value), dict(zip(("size", "windows", "blocks", "borrowed", "rounds", "fallback"), stats))


def check(emu, name, z, st, data, used, cap=None, **kw):
    """the wave-per-block reader against expand()'s verdict (st, data, used) and against the one-wave reader, field by field"""
    cap = (len(data) if st == 0 else BIG) if cap is None else cap
    got, stats = run(emu, z, cap, **kw)
    ref, _ = run(emu, z, cap, one=True, mis=kw.get("mis", 0), omis=kw.get("omis", 0))
    assert got == ref, (name, got[:3], ref[:3])
    assert got[0] == st and got[3] == data, (name, got[0], st)
    if st == 0:
        assert got[2] == used, name
    return stats


def test_frame_xxh64_against_the_writer(emu):
    """the frame checksum's fold (sixteen stripes loaded ahead) around its 512-byte trips and the 32-byte stripes"""
    emu.emul_zstd_large_xxh64_low.restype = C.c_uint32
    emu.emul_zstd_large_xxh64_low.argtypes = [C.c_char_p, C.c_uint32]
    d = zf.text(5000, 31)
    for n in (0, 1, 31, 32, 511, 512, 513, 543, 544, 575, 1023, 1024, 1025, 1055, 1056, 1535, 1536, 4999, 5000):
        assert emu.emul_zstd_large_xxh64_low(d[:n], n) == zf.xxh64(d[:n]) & 0xFFFFFFFF, n


def test_every_case(emu):
    """the multi-block cases at both windows: every field, and the counters -- all blocks by waves of their own, the dependent
    ones counted, no fallback on a valid stream but the one over the block cap (2), a fallback on every failing one (1)"""
    cases = zc.cases()
    assert len(cases) >= 35 and sum(1 for c in cases if c[2] != 0) >= 10
    for w in WINDOWS:
        for k, (name, z, st, data, used, blocks, borrowed) in enumerate(cases):
            s = check(emu, name, z, st, data, used, window=w, seed=k + 1)
            if zc.over_cap(name):
                assert st == 0 and s["fallback"] == 2, name
            elif st == 0:
                assert s["fallback"] == 0 and s["blocks"] == blocks and s["borrowed"] == borrowed, (name, s, blocks, borrowed)
                if w and len(data) > 2 * zf.BLOCK_MAX:
                    assert s["windows"] >= 3, (name, s)
            else:
                assert s["fallback"] == 1, (name, s)


def test_window_seams_fall_between_dependent_blocks(emu):
    """at 4096 bytes per window the chains are cut many times: a window's history is what the windows before it resolved"""
    by = dict((c[0], c) for c in zc.cases())
    for name in ("treeless_chain_39_s1_fse0", "rep_ten_blocks_of_repeat_codes", "copy_chain_64_blocks"):
        _, z, st, data, used, blocks, borrowed = by[name]
        s = check(emu, name, z, st, data, used, window=1)       # (a window holds one block at least: here exactly one)
        assert s["windows"] == blocks and s["fallback"] == 0, (name, s)
        s = check(emu, name, z, st, data, used, window=0)
        assert s["windows"] == 1 and s["rounds"] >= 2, (name, s)


def test_dependent_blocks_are_counted(emu):
    by = dict((c[0], c) for c in zc.cases())
    assert by["treeless_chain_39_s1_fse0"][5:] == (40, 39)
    assert by["repeat_each_table_another_definer"][5:] == (6, 4)
    assert by["copy_chain_64_blocks"][5:] == (65, 0)
    assert by["treeless_tree_redefined"][5:] == (12, 10)


def test_every_program_of_zstd_frames(emu):
    """all program families of zstd_frames (mostly one block): the fields are the one-wave reader's; a valid one never falls back"""
    for w in WINDOWS:
        for k, (name, z, st, data, used) in enumerate(zf.verdicts()):
            s = check(emu, name, z, st, data, used, window=w, seed=k)
            assert (s["fallback"] == 0) == (st == 0), (name, s)
            if st == 0:
                assert (s["blocks"], s["borrowed"]) == zc.census(z), name


def test_compressor_output(emu):
    for k, (name, z, d) in enumerate(zf.payloads()):
        s = check(emu, name, z, 0, d, len(z), mis=k % 5, omis=(3 * k) % 7, window=WINDOWS[k % 2])
        assert s["fallback"] == 0 and (s["blocks"], s["borrowed"]) == zc.census(z), (name, s)
        s = check(emu, name, z + b"tail", zf.DATA_ERROR, d, 0, cap=len(d))
        assert s["fallback"] == 1, name


@pytest.mark.skipif(zf.LIBZSTD is None, reason="libzstd does not load")
def test_libzstd_multi_block(emu):
    """1 MiB of prose / text at levels 1 / 3 / 19 (8 blocks, most of them with treeless literals) and flushed streams"""
    borrowed = 0
    for gen in (zf.prose, zf.text):
        d = gen(1 << 20, 41)
        for lvl in (1, 3, 19):
            z = zf.compress(d, lvl, checksum=lvl != 1)
            for w in (0, 300000):
                s = check(emu, "%s_l%d" % (gen.__name__, lvl), z, 0, d, len(z), window=w, seed=lvl)
                assert s["fallback"] == 0 and (s["blocks"], s["borrowed"]) == zc.census(z) and s["blocks"] >= 8, s
                assert s["windows"] == (1 if w == 0 else 4), s
            borrowed += s["borrowed"]
    assert borrowed >= 6
    d = zf.text(60000, 43)
    for piece in (150, 1000, 7777):
        z = zf.compress_flushed(d, piece)
        s = check(emu, "flushed_%d" % piece, z, 0, d, len(z), window=4096, mis=piece % 16)
        assert s["fallback"] == 0 and s["blocks"] == zc.census(z)[0] >= 60000 // piece, s


@pytest.mark.parametrize("mis", range(16))
def test_misaligned(emu, mis):
    """misalignments 0 .. 15 on both sides"""
    cases = [c for c in zc.cases() if len(c[1]) < 20000][mis % 3::3]
    for k, (name, z, st, data, used, blocks, borrowed) in enumerate(cases):
        check(emu, name, z, st, data, used, mis=mis, omis=(mis * 7 + k) % 16, window=WINDOWS[k % 2], seed=mis)


def test_out_cap_one_short(emu):
    """out_cap one short gives the one-wave status (-200) and its prefix; 0 bytes of room as well"""
    cases = [c for c in zc.cases() if c[2] == 0 and 0 < len(c[3]) and not zc.over_cap(c[0])]
    assert len(cases) >= 20
    for k, (name, z, st, data, used, blocks, borrowed) in enumerate(cases):
        want = zf.expand(z, len(data) - 1)
        s = check(emu, name, z, want[0], want[1], want[2], cap=len(data) - 1, window=WINDOWS[k % 2])
        assert want[0] == zf.OUT_FULL and s["fallback"] == 1, name
        want = zf.expand(z, 0)
        check(emu, name, z, want[0], want[1], want[2], cap=0)
        s = check(emu, name, z, st, data, used, cap=len(data) + 37, window=WINDOWS[(k + 1) % 2])
        assert s["fallback"] == 0, name


def test_order_of_blocks_does_not_matter(emu):
    by = dict((c[0], c) for c in zc.cases())
    for name in ("treeless_between_other_blocks", "rep_pushes_0_1_2", "frames_with_skippables"):
        for seed in range(1, 9):
            check(emu, name, *by[name][1:5], window=WINDOWS[seed % 2], seed=1000 * seed)


def test_sanitised_standalone_program(tmp_path):
    """the same passes from a program of its own under -fsanitize=address,undefined: cases, programs and payloads dumped to
    files, exact-size heap buffers (input, output, source map)"""
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "emul_zstd_large_san")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DEMUL_ZSTD_LARGE_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe], check=True)
    chosen = [c[:5] for c in zc.cases() if not zc.over_cap(c[0])] + list(zf.verdicts()) + [(name, z, 0, d, len(z)) for name, z, d in zf.payloads()]
    args, want = [], []
    for k, (name, z, st, data, used) in enumerate(chosen):
        f = tmp_path / ("%03d.zst" % k)
        f.write_bytes(z)
        for cap, w in (((len(data), 0), (len(data), 4096), (max(len(data) - 1, 0), 4096)) if st == 0 else ((BIG, 0), (BIG, 4096))):
            args += [str(f), str(cap), str(w)]
            want.append((name, cap, st, data, used))
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    assert len(lines) >= len(want)
    for (name, cap, st, data, used), line in zip(want, lines):
        got = [int(x) for x in line.split()]
        if st == 0 and cap == len(data):
            assert got[:5] == [0, len(data), used, zlib.crc32(data), 0], name
        elif st == 0:
            assert got[0] == (zf.OUT_FULL if data else 0), name
        else:
            assert got[0] == st and got[1] == len(data) and got[3] == zlib.crc32(data) and got[4] == 1, (name, got, st)
