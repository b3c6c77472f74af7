"""CPU tests of minizip-ng_amd/csrc/zstd_core.h through its host build (tests/emul/emul_zstd.cpp, g++ -DMZHIP_HOST_EMUL):
every program family of tests/zstd_frames.py and libzstd's streams, against the verdicts of expand() -- status, out_len,
in_used, bytes and CRC-32 exact.  Entries sit inside patterned buffers with red zones at several misalignments, and run one
after the other through ONE wave's LDS and scratch.  Counters that exist in the emulation only (-DMZ_ZS_STATS) hold each
family to its name.  The product path is the HIP build of the same header (tests/test_gpu_zstd.py)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import zstd_frames as zf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minizip-ng_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emul", "emul_zstd.cpp")
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
RED = 256
BIG = 400000   # an out_cap that no program fills

# the fields of mz_zs_stats (zstd_core.h), in its order
STAT_FIELDS = (("lit", 16), ("mode", 12), ("ll_code", 36), ("ml_code", 53), ("of_code", 32), ("rep_rule", 7), ("overlap", 72),
               ("weights_direct", 1), ("weights_fse", 1), ("streams1", 1), ("streams4", 1), ("treeless", 1), ("frames", 1),
               ("skippable", 1), ("checksums", 1), ("less_than_one", 1), ("zero_repeat3", 1))


def build_emul():
    """the host build of the core as a shared library, loaded"""
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libemul_zstd.so")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DMZ_ZS_STATS", "-I" + CSRC, "-shared", "-fPIC", SRC,
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.emul_zstd_wave_new.restype = C.c_void_p
    L.emul_zstd_wave_free.argtypes = [C.c_void_p]
    L.emul_zstd_run.restype = C.c_int32
    L.emul_zstd_run.argtypes = [C.c_void_p, _u8p, C.c_uint32, _u8p, C.c_uint32, _u32p, _u32p, _u32p]
    L.emul_zstd_stats.restype = C.c_uint32
    L.emul_zstd_stats.argtypes = [_u32p, C.c_uint32, C.c_int]
    L.emul_zstd_lds_bytes.restype = C.c_uint32
    L.emul_zstd_scratch_bytes.restype = C.c_uint32
    L.emul_zstd_xxh64_low.restype = C.c_uint32
    L.emul_zstd_xxh64_low.argtypes = [C.c_char_p, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def emu():
    return build_emul()


@pytest.fixture()
def wave(emu):
    w = emu.emul_zstd_wave_new()
    yield w
    emu.emul_zstd_wave_free(w)


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
    st = emu.emul_zstd_run(wave, C.cast(a.ctypes.data + i0, _u8p), len(z), C.cast(out.ctypes.data + o0, _u8p), cap,
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
    """expand()'s verdict (st, data, used) against the core's: the bytes of the complete blocks also where the stream fails"""
    got = run(emu, wave, z, (len(data) if st == 0 else BIG) if cap is None else cap, mis, omis)
    assert got[0] == st, (name, got[0], st)
    assert got[1] == len(data) and got[3] == data and got[4] == zlib.crc32(data), name
    if st == 0:
        assert got[2] == used, name


def stats(emu, reset=True):
    n = sum(k for _, k in STAT_FIELDS)
    buf = (C.c_uint32 * n)()
    assert emu.emul_zstd_stats(buf, n, int(reset)) == n
    out, p = {}, 0
    for name, k in STAT_FIELDS:
        out[name] = list(buf[p:p + k]) if k > 1 else int(buf[p])
        p += k
    return out


def test_layout_fits_the_launch(emu):
    assert emu.emul_zstd_lds_bytes() + 1024 <= 160 * 1024 // 8      # 8 single-wave workgroups per CU, each with the CRC byte table
    assert emu.emul_zstd_scratch_bytes() >= 128 * 1024 and emu.emul_zstd_scratch_bytes() % 256 == 0


def test_xxh64_against_the_writer(emu):
    d = zf.text(700, 31)
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 95, 96, 700):
        assert emu.emul_zstd_xxh64_low(d[:n], n) == zf.xxh64(d[:n]) & 0xFFFFFFFF, n
    assert zf.xxh64(b"") == 0xEF46DB3751D8E999     # the published value of XXH64 of nothing, seed 0


def test_every_program_one_wave(emu, wave):
    """all families, one behind the other through one wave's state, out_cap exactly the length for the valid ones"""
    for name, z, st, data, used in zf.verdicts():
        expect(emu, wave, name, z, st, data, used)
    for name, z, st, data, used in reversed(zf.verdicts()):
        expect(emu, wave, name, z, st, data, used, cap=(len(data) + 37) if st == 0 else BIG)


@pytest.mark.parametrize("mis,omis", [(0, 0), (1, 3), (2, 1), (3, 2), (7, 15), (13, 5)])
def test_programs_misaligned(emu, wave, mis, omis):
    for name, z, st, data, used in zf.verdicts()[(mis % 3)::3]:
        if len(z) < 20000:
            expect(emu, wave, name, z, st, data, used, mis=mis, omis=omis)


def test_compressor_output(emu, wave):
    for k, (name, z, d) in enumerate(zf.payloads()):
        expect(emu, wave, name, z, 0, d, len(z), mis=k % 5, omis=(3 * k) % 7)
        st, ol, iu, got, _ = run(emu, wave, z + b"tail", len(d), mis=(k + 1) % 4)
        assert (st, got) == (zf.DATA_ERROR, d), name             # stray bytes behind the last frame: an unknown magic
        assert run(emu, wave, z + b"\x28", len(d))[0] == zf.BUF_ERROR, name


def test_out_cap_one_short(emu, wave):
    """out_cap one short is -200 and what stands is a prefix; 0 bytes of room as well"""
    cases = [v for v in zf.verdicts() if v[2] == 0 and 0 < len(v[3]) <= 5000][::4] + [(n, z, 0, d, len(z)) for n, z, d in zf.payloads() if d]
    assert len(cases) >= 60
    for k, (name, z, st, data, used) in enumerate(cases):
        got = run(emu, wave, z, len(data) - 1, omis=k % 3)
        assert got[0] == zf.OUT_FULL and data.startswith(got[3]), name
        assert got[1] == len(zf.expand(z, len(data) - 1)[1]), name
        assert run(emu, wave, z, 0)[0] == zf.OUT_FULL, name


def test_first_problem_decides(emu, wave):
    T = zf.text(700, 5)
    f = zf.Frame(checksum=True, checksum_xor=1)
    f.content = T
    z = f.raw(T[:300]).comp(T[300:], lit_mode="huf").bytes()
    assert run(emu, wave, z, 299)[:2] == (zf.OUT_FULL, 0)              # the first block does not fit
    assert run(emu, wave, z, 699)[:2] == (zf.OUT_FULL, 300)            # the second does not: the first stands
    assert run(emu, wave, z, 700)[:2] == (zf.DATA_ERROR, 700)          # the checksum behind both is wrong
    assert run(emu, wave, z[:-2], 700)[:2] == (zf.BUF_ERROR, 700)      # ... or cut
    assert run(emu, wave, b"", 16)[:3] == (zf.BUF_ERROR, 0, 0)


def _kinds():
    pick = ("three_blocks_300k", "weights_fse_256_symbols", "lit_huf4_sf3_131072", "treeless_after_tree", "mode_0_rep_after_fse",
            "huf_length_11", "al_0_9", "al_2_9", "al_1_8", "zero_repeat_chain_1", "copy_distance_7", "block_rle_128k", "treeless_no_tree",
            "mode_1_rep_nothing", "weights_incomplete", "huf_bits_left_over", "cut_09", "skippable_only", "empty_frame")
    kinds = [v for v in zf.verdicts() if v[0] in pick]
    assert len(kinds) == len(pick)
    return kinds


def test_each_kind_behind_each_other_kind(emu, wave):
    """what an entry leaves in LDS and scratch -- a tree, tables at the largest accuracy logs, 128 KiB of literals, an error
    half-way -- must not reach the next entry: "treeless" and "repeat" find nothing to repeat in a new frame"""
    kinds = _kinds()
    for a in kinds:
        for b in kinds:
            if len(a[1]) > 20000 and len(b[1]) > 20000:
                continue
            expect(emu, wave, a[0], *a[1:])
            expect(emu, wave, a[0] + " -> " + b[0], *b[1:])


def test_families_are_what_their_names_say(emu, wave):
    """the counters of the emulation: every literals type and size format, every mode per table, every code, every
    repeat-offset rule, an overlapping copy at every distance 1 .. 70"""
    def only(prefix):
        stats(emu)
        for v in zf.verdicts():
            if v[0].startswith(prefix):
                run(emu, wave, v[1], BIG)
        return stats(emu)

    s = only("lit_")
    assert all(s["lit"][k] > 0 for k in range(12))        # Raw, RLE and Compressed literals x the four size formats
    assert s["streams1"] > 0 and s["streams4"] > 0
    s = only("weights_")
    assert s["weights_direct"] >= 2 and s["weights_fse"] >= 2
    s = only("treeless_")
    assert s["treeless"] >= 4 and all(s["lit"][k] > 0 for k in range(12, 16))
    s = only("mode_")
    assert all(x > 0 for x in s["mode"])
    for t in range(3):
        s = only("mode_%d_rep_after" % t)
        assert s["mode"][4 * t + 3] == 3
    s = only("ll_code_")
    assert all(x > 0 for x in s["ll_code"])
    s = only("ml_code_")
    assert all(x > 0 for x in s["ml_code"])
    s = only("of_code")
    assert all(x > 0 for x in s["of_code"])
    for ofv in (1, 2, 3):
        for k, ll in ((0, 2), (3, 0)):
            s = only("rep_%d_ll%d" % (ofv, ll))
            assert s["rep_rule"][ofv + k] >= 3
    for d in range(1, 71):
        s = only("copy_distance_%d" % d)
        assert s["overlap"][d] > 0, d
    s = only("less_than_one_")
    assert s["less_than_one"] >= 3
    s = only("zero_repeat_chain_")
    assert s["zero_repeat3"] >= 3 * 4
    s = only("skippable_")
    assert s["skippable"] >= 32
    s = only("checksum_")
    assert s["checksums"] >= 11


def test_reference_seed_archive(emu, wave):
    """the reference's fuzzer seed license_zstd.zip: one real zstd frame under the obsolete method number 20"""
    raw = open(os.path.join(ROOT, "tests", "golden", "license_zstd.zip"), "rb").read()
    assert len(raw) == 734 and raw[:4] == b"PK\x03\x04" and int.from_bytes(raw[8:10], "little") == 20
    cd = raw.index(b"PK\x01\x02")
    crc, csize, usize = (int.from_bytes(raw[cd + k:cd + k + 4], "little") for k in (16, 20, 24))
    p = 30 + int.from_bytes(raw[26:28], "little") + int.from_bytes(raw[28:30], "little")
    z = raw[p:p + csize]
    st, data, used = zf.expand(z)
    assert (st, len(data), used, zlib.crc32(data)) == (0, 894, csize, crc) and usize == 894
    expect(emu, wave, "license", z, 0, data, used, mis=p % 16)


def test_sanitised_standalone_program(tmp_path):
    """the same core from a program of its own under -fsanitize=address,undefined: every program and payload dumped to files,
    exact-size heap buffers, one wave for all of them"""
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "emul_zstd_san")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DEMUL_ZSTD_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe], check=True)
    chosen = list(zf.verdicts()) + [(name, z, 0, d, len(z)) for name, z, d in zf.payloads()]
    args, want = [], []
    for k, (name, z, st, data, used) in enumerate(chosen):
        f = tmp_path / ("%03d.zst" % k)
        f.write_bytes(z)
        for cap in ((len(data), max(len(data) - 1, 0)) if st == 0 else (BIG,)):
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
            assert got[0] == (zf.OUT_FULL if data else 0), name
        else:
            assert got[0] == st and got[1] == len(data) and got[3] == zlib.crc32(data), (name, got, st)
