"""CPU tests of the frame programs (tests/xz_frames.py): .xz streams whose framing fields are written one by one.

First the writer is held against the judge, liblzma (Python's lzma): a default-written frame decodes to its data, an
encoder-written image survives split() / write() byte for byte, and every named program gets the verdict its family names.
Then every named program and 6000 re-sealed mutations go through the host emulation of the device's container walk
(xz_core.h mz_xz_entry) and through the restatement (oracle/xz_dec.c): status, bytes, lengths, consumed input and CRC-32 as
liblzma gives them.  Where the mock drop-in and the compiled reference are built, the same programs are read through
mz_stream_lzma (method 95) on both, in whole, 7-byte and 1-byte read() calls, with the window knob off and at 4096 (the knob's
floor is 128 KiB: streams this small stay in one buffer either way), and streams of two 150 KB blocks through 128 KiB windows.
The last test runs the named programs through the same read() path in a program of its own under AddressSanitizer."""
import collections
import ctypes as C
import lzma
import os
import subprocess
import zlib

import pytest

import oracle
from tests import xz_frames as F
from tests.test_kernel_emul import _run, _u8p, emu  # noqa: F401  (emu: the module-scoped fixture that builds the emulation)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "emul", "_build", "libmockdrop.so")
SEED, N_RESEALED, N_STREAMED = 1, 6000, 700
CAP_REFUSED = 4096


def all_cases():
    """(name, stream, status, data, in_used): the named programs and the re-sealed set, as liblzma judged them"""
    return F.verdicts() + [r[:5] for r in F.resealed_verdicts(SEED, N_RESEALED)]


# ---- the writer against the judge ----------------------------------------------------------------------------------------
def test_default_frame_decodes():
    for check in F.VERIFIED:
        s = F.Stream([F.Block(F.A), F.Block(b""), F.Block(F.B, csize=True, usize=True)], check=check)
        assert lzma.decompress(s.write(), format=lzma.FORMAT_XZ) == F.A + F.B == s.data()
        assert F.judge(s.write() + b"more") == (0, len(s.write()), F.A + F.B)


def test_split_and_write_back():
    """an image from lzma.compress, split with the reader and written back, is the same bytes: the writer's layout is the
    encoder's"""
    for check in (lzma.CHECK_NONE, lzma.CHECK_CRC32, lzma.CHECK_CRC64, lzma.CHECK_SHA256):
        for d in (b"", b"a", F.T, bytes(70000)):
            x = lzma.compress(d, format=lzma.FORMAT_XZ, check=check)
            assert F.split(x).write() == x, (check, len(d))
    x = lzma.compress(F.T, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_DELTA, dist=4), dict(id=lzma.FILTER_X86, start_offset=16),
                                                          dict(id=lzma.FILTER_LZMA2, preset=1)])
    assert F.split(x).write() == x
    # ... and a frame of this writer's with every optional field in it
    x = F.Stream([F.Block(F.A, csize=True, usize=True, hpad=7), F.Block(F.B, usize=True)], check=7).write()
    assert F.split(x).write() == x


def test_named_programs_get_their_family_s_verdict():
    per = collections.Counter()
    for (name, x, family, data), (_, _, st, out, used) in zip(F.programs(), F.verdicts()):
        assert st == F.STATUS[family], (name, family, st)
        per[(name.split("/")[0], family)] += 1
        if st == 0:
            assert out == data, name
            assert used == (len(x) - 14 if name.startswith("trailing/") else len(x)), name
        if st == F.BUF_ERROR:
            assert used == len(x)
        assert len(x) < 8192, (name, len(x))
    print(sorted(per.items()))
    fam = collections.Counter(k[0] for k in per.elements())
    assert min(fam[f] for f in ("sizes", "header", "checks", "padding", "index", "footer", "stream-header")) >= 4
    assert fam["prefix"] >= 500 and fam["trailing"] >= 40


def test_resealed_set_is_not_hollow():
    """the shares the re-sealed set must keep: enough mutants liblzma accepts, enough it wants more input for, and refusals
    from every zone -- a generator that drifted into "everything refused at the first CRC" would pass the comparisons below
    and test nothing"""
    R = F.resealed_verdicts(SEED, N_RESEALED)
    n = collections.Counter(r[2] for r in R)
    zones = collections.Counter(z for r in R if r[2] == F.DATA_ERROR for z in r[5])
    print("re-sealed: %s; refused by zone %s" % (dict(n), dict(zones)))
    assert len(R) == N_RESEALED and len(set(r[1] for r in R)) > N_RESEALED // 4
    assert n[0] >= 0.03 * N_RESEALED and n[F.BUF_ERROR] >= 0.01 * N_RESEALED
    assert all(zones[z] >= 1 for z in F.ZONES), zones
    assert max(len(r[1]) for r in R) < 8192
    assert {r[1][7] & 15 for r in R if r[2] == 0} >= {0, 1, 4, 10, 7}


# ---- the container walks against the judge -------------------------------------------------------------------------------
def _cap(st, data):
    return len(data) if st == 0 else CAP_REFUSED


def test_emulation_agrees_with_liblzma(emu):
    n = collections.Counter()
    part = F.partials()
    for i, (name, x, st, data, used) in enumerate(all_cases()):
        cap = _cap(st, data)
        got, iu, out, crc = _run(emu.emul_xz, x, cap, C.c_int64(-1), mis=i & 3, omis=(i >> 2) & 3)
        assert got == st, (name, got, st)
        if st == 0:
            assert (iu, out, crc) == (used, data, zlib.crc32(data)), (name, iu, used, len(out), len(data))
        elif st == F.BUF_ERROR:
            assert iu == len(x), (name, iu, len(x))
            assert name not in part or out == part[name], (name, len(out), len(part[name]))  # (a cut filtered block: what liblzma's chain released)
        assert crc == zlib.crc32(out), name
        n[st] += 1
    assert n[0] >= 300 and n[F.DATA_ERROR] >= 5000 and n[F.BUF_ERROR] >= 1000, n


def test_out_cap_one_less_is_out_full_in_the_emulation(emu):
    k = 0
    for name, x, st, data, used in all_cases():
        if st == 0 and len(data) > 0:
            got, iu, out, crc = _run(emu.emul_xz, x, len(data) - 1, C.c_int64(-1))
            assert got == F.OUT_FULL and data.startswith(out) and crc == zlib.crc32(out), (name, got)
            k += 1
    assert k >= 300


def test_restatement_agrees_with_liblzma():
    part = F.partials()
    for name, x, st, data, used in all_cases():
        so, uo, oo = oracle.xz_decode(x, _cap(st, data))
        assert so == st, (name, so, st)
        if st == 0:
            assert (uo, oo) == (used, data), name
        elif st == F.BUF_ERROR:
            assert uo == len(x), name
            assert name not in part or oo == part[name], (name, len(oo), len(part[name]))


# ---- mz_stream_lzma, method 95: the mock drop-in against the compiled reference -------------------------------------------
KEYS = ("rets", "out", "total_out", "close", "open")


def stream_cases(n_resealed):
    return F.verdicts() + [r[:5] for r in F.resealed_verdicts(SEED, N_RESEALED)[:n_resealed]]


def read_modes(x, size):
    """the ways a stream is read: whole reads, 7 bytes and one byte at a time, and with the limits mz_zip sets for an entry
    (TOTAL_IN_MAX = the compressed size; TOTAL_OUT_MAX = the size of the data the stream was written around, where known)"""
    modes = [dict(), dict(chunk=7), dict(chunk=1)]
    if len(x):
        modes.append(dict(max_in=len(x)) if size is None else dict(max_in=len(x), max_out=size))
    return modes


def window_cases():
    return F.verdicts(F.window_programs)


def window_modes(x, size):
    """streams of several windows: with mz_zip's limits (window mode from the first byte), without (the one-buffer path gives
    up at a window's worth), in reads that end exactly where the first block ends, and in small odd ones"""
    return [dict(max_in=len(x), max_out=size), dict(), dict(chunk=150000), dict(chunk=7777), dict(chunk=50000, max_in=len(x), max_out=size)]


def compare_streams(hip, ref, cases, windows=(0, 4096), modes=read_modes):
    """every case through stream_decode(95) on both libraries: the read() sequence, the bytes, TOTAL_OUT and close() equal.
    TOTAL_IN and the liblzma code behind error() are not promised for framing errors ("Method 95: what a
    refused container leaves behind"): they are compared for accepted streams and for streams that break off (liblzma wants
    more input), not for refused ones.  -> {class: number of differing runs}"""
    L = hip.L
    L.mzhip_set_stream_window.argtypes = [C.c_int64, C.c_int64]
    L.mzhip_set_stream_window.restype = None
    diffs, first = collections.Counter(), {}
    sizes = {name: len(d) for name, _, _, d in F.programs() + F.window_programs() if d is not None}
    try:
        for win in windows:
            L.mzhip_set_stream_window(win, 4096 if win else 0)
            for name, x, st, data, used in cases:
                cap = (len(data) if st == 0 else max(CAP_REFUSED, sizes.get(name, 0))) + 64
                for kw in modes(x, len(data) if st == 0 else sizes.get(name)):
                    a = hip.stream_decode(95, x, cap, **kw)
                    b = ref.stream_decode(95, x, cap, **kw)
                    same = all(a[k] == b[k] for k in KEYS) and (a["error"] != 0) == (b["error"] != 0)
                    if st == 0:
                        same = same and a["out"] == data and (a["total_in"], a["error"]) == (b["total_in"], b["error"]) == (used, 0)
                    elif st == F.BUF_ERROR:
                        same = same and (a["total_in"], a["error"]) == (b["total_in"], b["error"])
                    if not same:
                        key = (name.split("/")[0], "window" if win else "one buffer", tuple(sorted(kw)))
                        diffs[key] += 1
                        first.setdefault(key, (name, a["rets"][-3:], b["rets"][-3:], len(a["out"]), len(b["out"]), a["close"], b["close"]))
    finally:
        L.mzhip_set_stream_window(0, 0)
    return diffs, first


@pytest.fixture(scope="module")
def libs():
    if os.path.isdir("/root/reference"):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True, capture_output=True)
    if not os.path.exists(MOCK) or not oracle.have_ref():
        pytest.skip("tests/emul/_build/libmockdrop.so / oracle/_ref/libmzref.so need the reference sources at build time")
    return oracle.MzDriver(MOCK), oracle.ref()


def test_stream_reads_match_the_reference(libs):
    """mz_stream_lzma READ of method 95 on the emulated device against the all-reference build: the named programs and 700
    re-sealed mutations, window knob off and at 4096, whole / 7-byte / 1-byte reads and mz_zip's limits.  A stream liblzma
    refuses must fail in the read() call in which liblzma fails it, with the bytes liblzma had handed out before: a block
    header it refuses before a byte of the block, a declared size where it is exhausted, and anything wrong behind a block's
    last bytes (padding, check, next header, index, footer) in the call that would have returned them."""
    hip, ref = libs
    diffs, first = compare_streams(hip, ref, stream_cases(N_STREAMED))
    for k in sorted(diffs):
        print(k, diffs[k], first[k])
    assert not diffs, (sum(diffs.values()), sorted(first.items())[:6])


def test_stream_reads_in_windows_match_the_reference(libs):
    """the container walk of window mode (shim_lzma.c xz_stream_*): streams of two large blocks, one framing defect each, read
    through a 128 KiB window -- the same read() sequences, bytes, TOTAL_OUT and close() as the all-reference build"""
    hip, ref = libs
    counter = getattr(hip.L, "mzmock_lzma2_windows", None)
    w0 = counter() if counter else 0
    for name, x, family, data in F.window_programs():
        assert F.judge(x)[0] == F.STATUS[family] and len(x) < 8192, name
    diffs, first = compare_streams(hip, ref, window_cases(), windows=(128 << 10,), modes=window_modes)
    for k in sorted(diffs):
        print(k, diffs[k], first[k])
    assert not diffs, (sum(diffs.values()), sorted(first.items())[:6])
    assert not counter or counter() - w0 >= 3 * len(window_cases())


def test_sanitised_stream_program(libs, tmp_path):
    """tests/emul/xz_stream_main.c, a program of its own, under AddressSanitizer with the mock drop-in built the same
    way: every named program (the prefixes in whole reads only) through mz_stream_lzma READ from a heap block of the
    stream's exact length, whole and in 7-byte reads, with and without mz_zip's limits.  The walk that places a refusal
    (shim_lzma.c xz_locate_refusal) reads chunk headers whose size fields an entry can set at will: a read behind the input
    it was given, or a write behind the bytes the device made, ends the child with a report.  What the runs return is what
    the all-reference build returns."""
    import struct

    _, ref = libs
    emul = os.path.join(ROOT, "tests", "emul")
    p = subprocess.run(["make", "-s", "-C", emul, "B=_build_asan", "SAN=address", "_build_asan/libmockdrop.so"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    exe = str(tmp_path / "xz_stream_main")
    subprocess.run(["gcc", "-O1", "-g", "-std=c99", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(emul, "xz_stream_main.c"), "-o", exe, "-L" + os.path.join(emul, "_build_asan"), "-lmockdrop",
                    "-Wl,-rpath," + os.path.join(emul, "_build_asan")], check=True)
    sizes = {name: len(d) for name, _, _, d in F.programs() if d is not None}
    cases = []
    for name, x, st, data, used in F.verdicts():
        size = len(data) if st == 0 else sizes.get(name)
        cases.append((name, x, (len(data) if st == 0 else max(CAP_REFUSED, sizes.get(name, 0))) + 64, size))
    blob = struct.pack("<I", len(cases)) + b"".join(struct.pack("<III", len(x), cap, 0xFFFFFFFF if size is None else size) + x
                                                     for _, x, cap, size in cases)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, p.stderr[-4000:]
    runs = 0
    for line in p.stdout.split("\n")[:-1]:
        c, chunk, lim, nr, last, produced, total_out, close, crc = (int(v) for v in line.split())
        name, x, cap, size = cases[c]
        if name.startswith("prefix/") and (chunk != 65535 or lim):
            continue
        kw = dict(chunk=chunk)
        if lim:
            kw.update(dict(max_in=len(x)) if size is None else dict(max_in=len(x), max_out=size))
        b = ref.stream_decode(95, x, cap, **kw)
        assert (nr, last, produced, total_out, close, crc) == (len(b["rets"]), b["rets"][-1], len(b["out"]), b["total_out"], b["close"],
                                                                zlib.crc32(b["out"])), (name, kw)
        runs += 1
    assert runs >= 4 * 200 + 800 and any("csize-behind-cut-chunk" in c[0] for c in cases)
