"""CPU tests of minizip-ng_amd/csrc/zstd_enc_core.h through its host build (tests/emul/emul_zstd_enc.cpp, g++
-DMZHIP_HOST_EMUL): the inputs of tests/zstd_enc_cases.py, judged for the round trip by the plain reader zf.expand(), by the
host build of the DECODER (emul_zstd.cpp) and, where it loads, by libzstd; and by the structural reader tests/zstd_tokens.py
for what the format and the header's contract fix: repeat offsets used wherever expressible, merged matches, one or four
Huffman streams, the tree description's form, code lengths, block types, the frame header, the checksum.  Entries sit inside
patterned buffers with red zones at several misalignments, and run one after the other through ONE wave's LDS and scratch.
The product path is the HIP build of the same header (tests/test_gpu_zstd_enc.py)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import synth
from tests import zstd_enc_cases as cs
from tests import zstd_frames as zf
from tests import zstd_tokens as zt

ROOT, CSRC, SRC = cs.ROOT, cs.CSRC, cs.EMUL_SRC
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
RED = 256
OUT_FULL, PARAM_ERROR = -200, -102
BLOCK = cs.BLOCK


@pytest.fixture(scope="module")
def emu():
    return cs.load_emul()


@pytest.fixture(scope="module")
def dec():
    L = C.CDLL(cs.build_emul("libemul_zstd.so", os.path.join(ROOT, "tests", "emul", "emul_zstd.cpp")))
    L.emul_zstd_wave_new.restype = C.c_void_p
    L.emul_zstd_wave_free.argtypes = [C.c_void_p]
    L.emul_zstd_run.restype = C.c_int32
    L.emul_zstd_run.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, _u32p, _u32p, _u32p]
    w = L.emul_zstd_wave_new()
    yield L, w
    L.emul_zstd_wave_free(w)


@pytest.fixture(scope="module")
def wave(emu):
    w = emu.emul_zstd_enc_wave_new()
    yield w
    emu.emul_zstd_enc_wave_free(w)


def _pattern(n, seed):
    return np.random.RandomState(seed).randint(1, 256, size=n, dtype=np.uint8)


def run(emu, wave, data, level, flags=0, cap=None, mis=0, omis=0):
    """one entry inside patterned buffers with red zones, at the byte misalignments mis / omis (relative to 16): the input is
    unchanged afterwards, nothing outside [out, out + cap) is written, and with status 0 nothing behind out_len.
    cap None = the bound.  -> (status, frame, crc)"""
    if cap is None:
        cap = int(emu.emul_zstd_enc_bound(len(data)))
    a = _pattern(RED + 16 + len(data) + RED, 311)
    i0 = RED + (-(a.ctypes.data + RED) % 16) + mis
    a[i0:i0 + len(data)] = np.frombuffer(data, dtype=np.uint8)
    a0 = a.copy()
    out = _pattern(RED + 16 + cap + RED, 312)
    o0 = RED + (-(out.ctypes.data + RED) % 16) + omis
    out0 = out.copy()
    ol, crc = C.c_uint32(0xFFFFFFFF), C.c_uint32(0x12345678)
    st = emu.emul_zstd_enc_run(wave, C.cast(a.ctypes.data + i0, _u8p), len(data), C.cast(out.ctypes.data + o0, _u8p), cap, level, flags,
                               C.byref(ol), C.byref(crc))
    assert (a == a0).all(), "input changed"
    assert ol.value <= cap
    keep = np.ones(out.size, dtype=bool)
    keep[o0:o0 + (ol.value if st == 0 else cap)] = False
    bad = np.flatnonzero((out != out0) & keep)
    assert bad.size == 0, "byte at offset %d of the output (status %d, out_len %d, cap %d) was written" % (int(bad[0]) - o0, st, ol.value, cap)
    if st != 0:
        assert ol.value == 0
    assert crc.value == zlib.crc32(data)
    return st, out[o0:o0 + ol.value].tobytes(), crc.value


def round_trip(name, z, data, dec=None):
    if len(data) <= 1 << 20:
        assert zf.expand(z) == (0, data, len(z)), name
    if zf.LIBZSTD is not None:
        assert zf.judge(z, len(data)) == ("valid", data), name
    if dec is not None:
        L, w = dec
        buf = C.create_string_buffer(max(len(data), 1))
        ol, iu, crc = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = L.emul_zstd_run(w, z, len(z), buf, len(data), C.byref(ol), C.byref(iu), C.byref(crc))
        assert (st, ol.value, iu.value, crc.value) == (0, len(data), len(z), zlib.crc32(data)), name
        assert buf.raw[:len(data)] == data, name


def expressible(ll, dist, rep):
    """the repeat value that names `dist` for a sequence with literal length ll behind the history rep, or None"""
    if ll:
        names = (rep[0], rep[1], rep[2])
    else:
        names = (rep[1], rep[2], rep[0] - 1)
    for v, d in enumerate(names):
        if d == dist and d != 0:
            return v + 1
    return None


def check_structure(name, z, data, flags):
    """what the format and zstd_enc_core.h's contract fix about the frame of `data`; -> the frame as zstd_tokens reads it"""
    frames = zt.read(z)
    assert len(frames) == 1 and frames[0]["size"] == len(z), name
    f = frames[0]
    n = len(data)
    assert f["did_bytes"] == 0 and f["fcs"] == n, name
    if n <= cs.FAR_DICT:
        assert f["single"] and f["window_byte"] is None and f["fcs_bytes"] == (1 if n < 256 else 2 if n < 65792 else 4), name
    else:
        assert not f["single"] and f["window"] == 8 << 20 and f["window_byte"] == 13 << 3 and f["fcs_bytes"] == 4, name
    assert f["checksum"] == bool(flags & 1), name
    if flags & 1:
        assert f["checksum_value"] == zf.xxh64(data) & 0xFFFFFFFF, name
    blocks = f["blocks"]
    assert len(blocks) == max(1, (n + BLOCK - 1) // BLOCK) and [b["last"] for b in blocks] == [False] * (len(blocks) - 1) + [True], name
    pos = 0
    for k, b in enumerate(blocks):
        want = data[pos:pos + BLOCK]
        if b["type"] == "rle":
            assert len(set(want)) == 1 and b["size"] == len(want), (name, k)
        elif b["type"] == "raw":
            assert b["size"] == len(want) and (len(want) == 0 or len(set(want)) > 1), (name, k)
        else:
            assert 3 <= b["size"] < len(want) and len(set(want)) > 1, (name, k, b["size"])
            li = b["literals"]
            assert li["mode"] in ("raw", "rle", "huf"), (name, k)
            if li["mode"] == "huf":
                assert li["max_code_len"] <= 11, (name, k)
                assert li["streams"] == (1 if li["regen"] <= 1023 else 4), (name, k, li["regen"])
                assert li["size_format"] == (0 if li["streams"] == 1 else 2 if li["regen"] < 16384 and li["comp"] < 16384 else 3), (name, k)
                assert li["header"] + li["comp"] < (1 if li["regen"] < 32 else 2 if li["regen"] < 4096 else 3) + li["regen"], (name, k)
                present = [s for s in range(256) if s in set(b["lits"])]
                assert [s for s, w in enumerate(li["weights"]) if w] == present, (name, k)
                direct = 1 + (present[-1] + 1) // 2       # a direct description lists the weights in front of the last value
                if li["tree"] == "fse":
                    assert present[-1] > 128 or li["tree_bytes"] < direct, (name, k, "FSE-compressed weights are taken when shorter")
                else:
                    assert present[-1] <= 128 and li["tree_bytes"] == direct, (name, k)
                w = li["weights"]
                assert sum(1 << (x - 1) for x in w if x) == 1 << li["max_code_len"] and w.count(1) >= 2, (name, k)
            elif li["mode"] == "rle":
                assert len(set(b["lits"])) == 1, (name, k)
            else:
                assert li["size_format"] == ((2 if li["regen"] & 1 else 0) if li["regen"] < 32 else 1 if li["regen"] < 4096 else 3), (name, k)
            assert b["nseq"] <= 16384 and b["count_form"] == (1 if b["nseq"] < 128 else 2), (name, k)
            if b["nseq"]:
                for t, (mode, al) in enumerate(zip(b["modes"], b["accuracy"])):
                    assert mode in ("predefined", "rle", "fse"), (name, k)
                    codes = set((zf.code_of(zf.LL_CODES, s[0]), zf.highbit(s[2]), zf.code_of(zf.ML_CODES, s[1]))[t] for s in b["sequences"])
                    assert (mode == "rle") == (len(codes) == 1), (name, k, t)
                    if mode == "fse":
                        assert 5 <= al <= (8 if t == 1 else 9), (name, k, t)
            at, prev = pos, None
            for ll, ml, ofv, dist, rep in b["sequences"]:
                assert ml >= 4 and at + ll + ml <= pos + len(want), (name, k)
                assert dist < (8 << 20) and (n > BLOCK or dist <= 32768), (name, k, dist)
                v = expressible(ll, dist, rep)
                assert (ofv if ofv <= 3 else None) == v, (name, k, (ll, ml, ofv, dist, rep))
                assert not (ll == 0 and prev == dist), (name, k, "two matches of one distance side by side were not merged")
                at, prev = at + ll + ml, dist
        pos += len(want)
    if n <= 1 << 20:
        assert zt.replay(frames) == data, name
    return f


def test_layout_fits_the_launch(emu):
    assert emu.emul_zstd_enc_lds_bytes() + 1024 <= 160 * 1024 // 8      # 8 single-wave workgroups per CU, each with the CRC byte table
    assert emu.emul_zstd_enc_scratch_bytes() == 65536 + 8 * 16384 + 65536 + 1024
    for n, blocks in ((0, 1), (1, 1), (65536, 1), (65537, 2), (1 << 20, 16)):
        assert emu.emul_zstd_enc_bound(n) == 14 + n + 3 * blocks


_STREAMS = {}


def streams(emu, wave):
    """{name: frame} of every case at the bound, through the one wave in list order, computed once: the reference the other
    tests compare with"""
    if not _STREAMS:
        emu.emul_zstd_enc_max_nseq(1)
        for name, data, level, flags in cs.cases():
            st, z, _ = run(emu, wave, data, level, flags)
            assert st == 0, name
            _STREAMS[name] = z
        assert 0 < emu.emul_zstd_enc_max_nseq(0) <= 16384
    return _STREAMS


def test_every_case_round_trips_one_wave(emu, wave, dec):
    """all inputs, one behind the other through one wave's state, then the smaller ones in reverse: the readers return the
    input, and the bytes do not depend on what the wave did before"""
    S = streams(emu, wave)
    for name, data, level, flags in cs.cases():
        round_trip(name, S[name], data, dec)
        assert len(S[name]) <= emu.emul_zstd_enc_bound(len(data)), name
    for name, data, level, flags in reversed(cs.cases()):
        if len(data) > 140000:
            continue
        st, z, _ = run(emu, wave, data, level, flags, mis=1, omis=3)
        assert st == 0 and z == S[name], name


def test_structure(emu, wave):
    S = streams(emu, wave)
    F = {}
    for name, data, level, flags in cs.cases():
        F[name] = check_structure(name, S[name], data, flags)

    def blocks(name):
        return F[name]["blocks"]

    def seqs(name, k=0):
        return blocks(name)[k]["sequences"]

    # an empty input: one empty Raw last block
    assert S["len_0"] == bytes.fromhex("28b52ffd2000010000") and [b["type"] for b in blocks("len_0")] == ["raw"]
    # block types
    assert [b["type"] for b in blocks("one_value_70000")] == ["rle", "rle"] and len(S["one_value_70000"]) == 4 + 1 + 4 + 2 * 4
    for k in (1000, 65536, 65538, 200000):
        name = "noise_%d" % k
        assert all(b["type"] == "raw" for b in blocks(name)), name
        assert len(S[name]) == k + F[name]["header_bytes"] + 3 * len(blocks(name)) + (4 if F[name]["checksum"] else 0), name
    assert [b["type"] for b in blocks("rep_across_raw_block")] == ["compressed", "raw", "compressed"]
    # literals
    assert blocks("one_value_literals")[0]["literals"]["mode"] in ("raw", "huf")
    assert (blocks("rle_literals")[1]["literals"]["mode"], blocks("rle_literals")[1]["lits"]) == ("rle", b"kkkkk")
    for k in (31, 32, 4095, 4096):
        li = blocks("raw_literals_%d" % k)[0]["literals"]
        assert (li["mode"], li["regen"]) == ("raw", k), k
    assert blocks("uniform_256")[0]["type"] == "raw" or blocks("uniform_256")[0]["literals"]["mode"] == "raw"
    for k, n_streams in ((1023, 1), (1024, 4)):
        b = blocks("streams_%d" % k)[0]
        assert (b["literals"]["mode"], b["literals"]["regen"], b["literals"]["streams"], b["nseq"]) == ("huf", k, n_streams, 0), k
    assert blocks("no_match_4096")[0]["nseq"] == 0 and blocks("no_match_4096")[0]["literals"]["streams"] == 4
    assert blocks("two_values")[0]["type"] == "compressed"
    for name, tree in (("low_values", "direct"), ("symbols_130", "fse"), ("bytes_high", "fse"), ("bytes_all", "fse")):
        li = blocks(name)[0]["literals"]
        assert (li["mode"], li["tree"]) == ("huf", tree), (name, li["mode"], li["tree"])
    for name, top in (("symbols_128", 127), ("symbols_129", 128)):             # (either form is legal here: check_structure holds the shorter one)
        li = blocks(name)[0]["literals"]
        assert li["mode"] == "huf" and max(blocks(name)[0]["lits"]) == top, name
    b = blocks("fibonacci_frequencies")[0]
    hist = [b["lits"].count(bytes([s])) for s in range(256)]
    assert max(zf.huf_lengths(hist, limit=99)) > 11 and b["literals"]["max_code_len"] <= 11      # the limit was needed, and held
    # sequence counts and their form
    assert [(blocks("nseq_%d" % k)[0]["nseq"], blocks("nseq_%d" % k)[0]["count_form"]) for k in (127, 128)] == [(127, 1), (128, 2)]
    # literal and match lengths
    assert [s[0] for s in seqs("literal_lengths")] == [400, 15, 16, 17, 1, 0]
    (ll, ml, _, dist, _), = seqs("literal_run_65000")
    assert ll > 65000 - 64 and ll + ml == 65200 and dist == 30000            # a literal length with 15 extra bits
    # (274 = 273 and a literal: a token holds 273.  277 and 546 are two tokens merged; the parse finds the last 327 of the
    # 600 elsewhere, which is its right)
    ml = [s[1] for s in seqs("match_lengths")]
    assert ml[:7] == [34, 35, 36, 273, 273, 277, 546] and sum(ml[7:]) == 600, ml
    assert [(s[1], s[3]) for s in seqs("match_run_60000")] == [(60000, 100)]                      # 220 tokens, one sequence
    for d in (1, 2, 3):
        first = seqs("distance_%d" % d)[0]
        assert (first[1], first[3]) == (273, d), d                         # a match longer than its distance
    # repeat offsets: the values written, in order
    assert [s[2] for s in seqs("rep_with_literals")][1:] == [1, 417 + 3, 2, 2, 533 + 3, 3]
    assert [s[2] for s in seqs("rep_without_literals")][1:] == [417 + 3, 1, 533 + 3, 3, 341 + 3, 2, 301 + 3, 3]
    v = [s[2] for s in seqs("rep_alternating")]
    assert v[:2] == [417 + 3, 301 + 3] and v.count(2) >= 30 and len(v) == 40      # (where the parse found another source, check_structure held the value)
    assert [(s[0], s[2]) for s in seqs("rep_across_seam", 1)] == [(5, 2), (30, 2)]
    assert blocks("rep_across_seam")[1]["rep_before"] == (700, 500, 20000)
    assert [(s[0], s[2]) for s in seqs("rep_across_raw_block", 2)] == [(5, 1), (30, 2)]
    # reach
    assert [s[3] for s in seqs("reach_32768")] == [32768]
    far = [s[3] for k in (1, 2, 3) for s in seqs("reach_100k_twice", k)]
    assert far and set(far) == {100 * 1024}


def test_window_descriptor_path(emu, wave, dec):
    """one entry longer than the far dictionary: a Window_Descriptor of exactly 8 MiB, a 4-byte content size, the checksum"""
    name, data, level, flags = cs.big()
    st, z, _ = run(emu, wave, data, level, flags)
    assert st == 0 and len(z) <= emu.emul_zstd_enc_bound(len(data))
    round_trip(name, z, data, dec)
    f = check_structure(name, z, data, flags)
    assert z[4] == 0x84 and z[5] == 0x68 and int.from_bytes(z[6:10], "little") == len(data) and f["header_bytes"] == 10
    assert len(z) < len(data) // 2


def test_levels_and_parameters(emu, wave):
    S = streams(emu, wave)
    size = dict((lv, len(S["levels_%d" % lv])) for lv in (1, 3, 9, 19, -1))
    assert S["levels_-1"] == S["levels_3"]                          # -1 means 3
    assert size[1] > size[3] >= size[9] >= size[19], size           # a deeper parse is never worse on prose
    data = cs.cases()[10][1]
    assert run(emu, wave, data, 0)[1] == run(emu, wave, data, 3)[1] and run(emu, wave, data, 22)[0] == 0
    out = (C.c_uint8 * 64)()
    for level in (23, -2, 100, -100):
        assert emu.emul_zstd_enc_run(wave, out, 0, out, 64, level, 0, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == PARAM_ERROR


@pytest.mark.parametrize("mis", range(16))
def test_small_cases_misaligned(emu, wave, mis):
    S = streams(emu, wave)
    for k, (name, data, level, flags) in enumerate(cs.small()):
        st, z, _ = run(emu, wave, data, level, flags, mis=mis, omis=(mis * 7 + k) % 16)
        assert st == 0 and z == S[name], name


def test_capacity_one_short(emu, wave):
    """out_cap exactly the size is enough; one byte less is the encoders' "does not fit", out_len 0, nothing outside the cap"""
    S = streams(emu, wave)
    for k, (name, data, level, flags) in enumerate(cs.cases()):
        if len(data) > 140000:
            continue
        z = S[name]
        st, z2, _ = run(emu, wave, data, level, flags, cap=len(z), omis=k % 16)
        assert st == 0 and z2 == z, name
        st, z2, _ = run(emu, wave, data, level, flags, cap=len(z) - 1, omis=(k + 5) % 16)
        assert st == OUT_FULL and z2 == b"", name
    assert run(emu, wave, b"", 3, cap=0)[0] == OUT_FULL
    assert run(emu, wave, cs.cases()[12][1], 3, cap=3)[0] == OUT_FULL


@pytest.mark.parametrize("size", [1, 255, 4096, 65536, 140000])
def test_bound_against_adversaries(emu, wave, size):
    rs = np.random.RandomState(size)
    noise = rs.bytes(size)
    one_match = bytearray(noise)                                     # noise with one long match per block
    for b0 in range(0, size, BLOCK):
        k = min(BLOCK, size - b0) // 3
        one_match[b0 + 2 * k:b0 + 3 * k] = one_match[b0:b0 + k]
    near_uniform = (rs.randint(0, 255, size=size)).astype(np.uint8).tobytes()      # 255 values, near-uniform
    for name, data in (("noise", noise), ("one_match", bytes(one_match)), ("near_uniform_255", near_uniform)):
        for level, flags in ((1, 0), (3, 1)):
            st, z, _ = run(emu, wave, data, level, flags)
            assert st == 0 and len(z) <= emu.emul_zstd_enc_bound(size), (name, level)
            round_trip(name, z, data)


# Output size against libzstd 1.4.8.  The encoder is deterministic, so the figures are exact; they were measured on the host
# build, which is the device's byte for byte (DESIGN section 3 "zstd encode" has the same table).  Bytes written, and the
# excess over libzstd at level 1 / at level 3:
#   corpus_64k   level 1   23 744   +5.39 %  / +10.93 %      level 3   21 301   -5.45 % /  -0.48 %
#   corpus_1m    level 1  137 631  +11.29 %  / +21.26 %      level 3  110 939  -10.29 % /  -2.26 %
#   markov_64k   level 1   30 592   +7.57 %  / +17.13 %      level 3   26 667   -6.23 % /  +2.11 %
#   markov_1m    level 1  316 881  -20.75 %  /  +2.27 %      level 3  270 022  -32.47 % / -12.85 %
# (level 1 is the one-candidate parse with one far link; libzstd's level 1 loses on markov_1m because its window is 512 KiB.)
# The bound for every input and both levels is libzstd level 1's size times (1 + m), m = the worst excess above, 11.29 %,
# rounded up to the next whole per cent.
SIZE_EXCESS_OVER_LEVEL1 = 0.12


def _size_inputs():
    T = synth.corpus()
    return [("corpus_64k", T[:BLOCK]), ("corpus_1m", (T * 3)[:1 << 20]), ("markov_64k", synth.markov_entries(1, BLOCK, seed=9)[0]),
            ("markov_1m", synth.markov_entries(1, 1 << 20, seed=9)[0])]


@pytest.mark.skipif(zf.LIBZSTD is None, reason="libzstd does not load")
def test_size_against_libzstd(emu, wave):
    for name, data in _size_inputs():
        ref1, ref3 = len(zf.compress(data, 1)), len(zf.compress(data, 3))
        for level in (1, 3):
            st, z, _ = run(emu, wave, data, level)
            print("%-12s level %d: %8d bytes; libzstd level 1 %8d (%+.2f %%), level 3 %8d (%+.2f %%)" %
                  (name, level, len(z), ref1, 100.0 * (len(z) - ref1) / ref1, ref3, 100.0 * (len(z) - ref3) / ref3))
            assert st == 0 and len(z) <= ref1 * (1 + SIZE_EXCESS_OVER_LEVEL1), (name, level, len(z), ref1)


def test_sanitised_standalone_program(tmp_path):
    """the same core from a program of its own under -fsanitize=address,undefined: inputs dumped to files, exact-size heap
    buffers (the bound, the size it took, one byte less), one wave for all of them"""
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "emul_zstd_enc_san")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DEMUL_ZSTD_ENC_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe], check=True)
    keep = ("streams_1023", "streams_1024", "symbols_130", "bytes_all", "fibonacci_frequencies", "nseq_128", "match_lengths", "raw_literals_4096",
            "noise_1000", "rep_alternating", "len_65537", "rep_across_raw_block")
    chosen = cs.small() + [c for c in cs.cases() if c[0] in keep]
    for level, flags in ((1, 0), (3, 1), (19, 0)):
        files = []
        for k, (name, data, _, _) in enumerate(chosen):
            f = tmp_path / ("%d_%03d.bin" % (level, k))
            f.write_bytes(data)
            files.append(f)
        r = subprocess.run([exe, str(level), str(flags)] + [str(f) for f in files], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        lines = r.stdout.split("\n")
        for (name, data, _, _), f, line in zip(chosen, files, lines):
            st, ol, crc, st_exact, st_short = [int(x) for x in line.split()]
            z = open(str(f) + ".zst", "rb").read()
            assert (st, ol, crc, st_exact, st_short) == (0, len(z), zlib.crc32(data), 0, OUT_FULL), (name, line)
            assert zf.expand(z) == (0, data, len(z)), name
