"""CPU tests of the header programs (tests/header_programs.py): the writer and the plain reader against zlib and the oracle
restatement, the capacity of the second-level table, what the families must hold, every program through the 64-lane emulation
of the device code -- the default build and the builds of test_kernel_emul.emu_staged --, the counters that show the 64-bit
front end, the serial loop behind it and the reads from memory behind the register window are all reached, and the many-wave
window through the host mock."""
import ctypes as C
import os
import random
import subprocess
import zlib

import pytest

import oracle
from tests import header_programs as H
from tests import token_programs as T
from tests.test_kernel_emul import ROOT, _build_variant, _run, emu, emu_staged  # noqa: F401  (the fixtures, built the same way)
from tests.test_token_programs import MOCK, emu_stats  # noqa: F401

CAP = 4096          # out_cap of the programs that produce nothing to compare: no program here stands for more


def _zlib_verdict(z, sentinel=b""):
    """-> (status class, bytes, unused input, zlib's message)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z + sentinel)
    except zlib.error as e:
        return -3, b"", b"", str(e)
    return (0 if d.eof else -5), out, d.unused_data, None


def test_writer_and_reader_against_the_judges():
    """Nothing else here may be believed until this passes.  For every accepted program zlib's raw inflate returns exactly the
    expected bytes and leaves exactly the sentinel byte appended behind the stream; every refused one it refuses with the message
    read_header() predicted (or, where the header is fine and the body is not, the one the program carries); every cut one
    it leaves unfinished, and read_header() says "input ended" when the cut lies inside the header.  The oracle restatement
    gives the same status class for every program and the same consumed count on success: a zlib build with other rules shows
    up here, as a disagreement between the two judges, and not later as a device failure."""
    print("zlib runtime version %s" % zlib.ZLIB_RUNTIME_VERSION)
    seen = {}
    for fam in H.ALL_FAMILIES:
        for name, prog, z, data in H.family(fam):
            bit = H.header_bit(prog)
            rh = H.read_header(z, bit)
            k, hdr = H.header_of(prog)
            st, out, unused, msg = _zlib_verdict(z, b"" if fam == "cut" else b"\x5a")
            so, uo, oo = oracle.inflate_raw(z, CAP)
            assert so == st, (name, so, st)
            if data is not None:
                assert (st, out, unused) == (0, data, b"\x5a"), (name, st, msg)
                assert (uo, oo) == (len(z), data), name
                lit, dist, end = rh
                assert (lit, dist) == T.spelled_lengths(hdr) and end == bit + H.header_bits(hdr), name
            elif fam == "cut":
                assert st == -5, (name, st, msg)
                if not isinstance(rh, str):
                    assert 8 * len(z) >= rh[2], name
                else:
                    assert rh == H.ENDED, (name, rh)
                seen[H.ENDED] = seen.get(H.ENDED, 0) + (rh == H.ENDED)
            else:
                want = rh if isinstance(rh, str) else hdr.get("refuse")
                assert st == -3 and want and want in msg, (name, st, msg, want)
                seen[want] = seen.get(want, 0) + 1
    print("verdicts: %s" % sorted(seen.items()))
    assert all(seen.get(r, 0) >= 4 for r in H.REASONS), seen
    assert seen[H.ENDED] >= 200


def test_second_level_capacity():
    """sub_entries() and worst_sub_code(): 404 entries behind an 8-bit root, 340 behind 9, 308 behind 10 -- the three values of
    MZ_LIT_SUB_ENTRIES in inflate_core.h --, reached by a code that is complete by Kraft's sum, has at most 286 symbols and 15
    bits; the counts the search was first run with (2 codes of 2 bits, 233 of 9, 45 of 10, one each of 11 .. 14, 2 of 15) need
    404 as well; zlib's own codes of a geometric source (synth.long_code_payloads) stay below it (260 where this was written)."""
    for root, want in ((8, 404), (9, 340), (10, 308)):
        lens = H.worst_sub_code(root)
        assert len(lens) <= 286 and max(lens) <= 15 and sum((1 << 15) >> l for l in lens) == 1 << 15, root
        assert H.sub_entries(lens, root) == want, (root, H.sub_entries(lens, root))
        rnd = random.Random(root)
        for _ in range(20):                                   # what a code needs does not depend on which symbol has which length ...
            mixed = list(lens)
            rnd.shuffle(mixed)
            assert H.sub_entries(mixed, root) == want
        for _ in range(200):                                  # ... and no neighbour of the worst code needs more
            other = sorted(lens)
            i = rnd.randrange(len(other))
            if other[i] < 15 and len(other) < 286:
                other[i:i + 1] = [other[i] + 1] * 2
            else:
                j = next((j for j in range(len(other) - 1) if other[j] == other[j + 1] and other[j] > 1 and rnd.random() < 0.05), None)
                if j is None:
                    continue
                other[j:j + 2] = [other[j] - 1]
            assert sum((1 << 15) >> l for l in other) == 1 << 15
            assert H.sub_entries(sorted(other), root) <= want, (root, other)
    named = [2] * 2 + [9] * 233 + [10] * 45 + [11, 12, 13, 14, 15, 15]
    assert len(named) == 286 and H.sub_entries(named, 8) == 404
    assert H.sub_entries([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, 8) == 112       # (the fixed code: 56 prefixes of two 9-bit codes)
    assert H.sub_entries([1, 2, 3, 3], 8) == 0
    from tests import synth

    most = 0
    for name, d, z in synth.long_code_payloads(size=20000):   # (the first block of each: a dynamic one)
        lit = H.read_header(z, 0)[0]
        assert max(lit) > 8, name
        most = max(most, H.sub_entries(lit, 8))
    print("second-level entries of zlib's own long codes: %d at the most, of 404" % most)
    assert 0 < most < 404


def _aligned_edge(prog):
    """bits from the header block's first bit to the end of the 2048-bit register window (input aligned to a dword)"""
    return 2048 - (H.header_bit(prog) & 31)


def test_families_hold_what_they_must():
    """The conditions on the families: 1 200 accepted programs, 300 refused, 200 cut, at most 4096 in all (one launch), streams
    below 2 KiB and expected outputs below 4 KiB; every HCLEN; every code-length symbol with a 1-bit and a 7-bit code among the
    operations; every extra value of 16, 17 and 18; runs that cross HLIT + 257 by every amount; the probe of `window` ending
    exactly at bit 64 of a front-end window and straddling it by 1 .. 13 bits, a 16 that is the first symbol of a window, an
    overrun in the middle of a window; the headers of `long` at every start bit modulo 32, up to the longest there is, with the
    end of the register window inside a plain length, inside the extra bits of a 16 and of an 18, and between two symbols."""
    acc = sum(e[3] is not None for f in H.FAMILIES for e in H.family(f))
    ref = sum(e[3] is None for f in H.FAMILIES for e in H.family(f))
    ncut = len(H.family("cut"))
    print("programs per family: %s; accepted %d, refused %d, cut %d"
          % ({f: len(H.family(f)) for f in H.ALL_FAMILIES}, acc, ref, ncut))
    assert acc >= 1200 and ref >= 300 and ncut >= 200 and acc + ref + ncut <= 4096
    for e in H.everything():
        assert len(e[2]) < 2048 and (e[3] is None or len(e[3]) < 4096), e[0]
    hdrs = {f: [(e[0], e[1], H.header_of(e[1])[1], e[3] is not None) for e in H.family(f)] for f in H.FAMILIES}
    good = lambda f: [h for h in hdrs[f] if h[3]]
    assert {h[2]["hclen"] + 4 for h in hdrs["clc"]} == set(range(4, 20))
    assert {h[2]["hclen"] + 4 for h in good("clc")} == set(range(5, 20))
    for s in range(19):
        for n in (1, 7):
            assert any(h[2]["cl"][s] == n and any(op[0] == s for op in h[2]["ops"]) for h in good("clc")), (s, n)
    for shape in H.CLC_SHAPES:
        assert any(sorted(l for l in h[2]["cl"] if l) == sorted(shape) for h in good("clc")), shape
    sent = {op for h in good("ops") for op in h[2]["ops"] if op[0] >= 16}
    assert sent >= {(16, x) for x in range(4)} | {(17, x) for x in range(8)} | {(18, x) for x in range(128)}
    crossing = set()                                             # (symbol, run, lengths of it that are distance lengths)
    zero16 = 0
    for name, prog, h, ok in good("ops"):
        nlen, at, before = h["hlit"] + 257, 0, None
        for s, x in h["ops"]:
            r = 1 if s < 16 else H.REP[s][1] + x
            if s >= 16 and at < nlen < at + r:
                crossing.add((s, r, at + r - nlen))
                if s == 16:
                    lit, dist = T.spelled_lengths(h)
                    assert lit[-1] == dist[0] != 0, name
            zero16 += s == 16 and before in (17, 18)
            at, before = at + r, s
    assert crossing >= {(16, r, c) for r in range(3, 7) for c in range(1, r)} | {(17, r, c) for r in range(3, 11) for c in range(1, r)}
    assert {(r, c) for s, r, c in crossing if s == 18} >= {(11, c) for c in range(1, 11)} | {(57, 28), (57, 29 - 1)}
    assert zero16 >= 8
    straddle, exact, first16, mid_overrun = set(), 0, 0, 0
    for name, prog, h, ok in hdrs["window"]:
        assert h["cl"][8] == 1 and h["cl"][16] == h["cl"][17] == h["cl"][18] == 7
        pad = int(name.rsplit("pad", 1)[1])
        wins = H.front_end_windows(h)
        if "refused" in name:                                   # the probe is the last operation: it overruns
            mid_overrun += wins[-1][1] > 0
            continue
        assert all(op == (8, 0) for op in h["ops"][:pad]), name
        w, off, n = wins[pad]                                   # the probe stands behind the pad operations, one bit each
        if pad + n <= 64:
            assert (w, off) == (0, pad), (name, w, off)
            exact += pad + n == 64
        elif pad < 64:                                          # it does not end inside the first window: it starts the second
            assert (w, off) == (1, 0), (name, w, off)
            straddle.add(pad + n - 64)
            first16 += h["ops"][pad][0] == 16
        else:
            assert (w, off) == (1, pad - 64), (name, w, off)
            first16 += h["ops"][pad][0] == 16 and pad == 64
    print("window: probe ends at bit 64 in %d programs, straddles it by %s, a 16 starts a window %d times, %d overruns in the middle of a window"
          % (exact, sorted(straddle), first16, mid_overrun))
    assert straddle == set(range(1, 14)) and exact >= 4 and first16 >= 2 and mid_overrun >= 300
    starts, kinds, longest = {}, set(), 0
    for name, prog, h, ok in hdrs["long"]:
        assert ok, name
        variant = name.split("/")[1]
        starts.setdefault(variant, set()).add(H.header_bit(prog) & 31)
        longest = max(longest, H.header_bits(h))
        edge, at = _aligned_edge(prog), H.ops_start(h)
        for s, x in h["ops"]:
            n = H.op_bits(h, (s, x))
            if at == edge:
                kinds.add("between")
            elif at < edge < at + n:
                kinds.add("plain" if s < 16 else "%d %s" % (s, "code" if edge <= at + h["cl"][s] else "extra"))
            at += n
    assert all(v == set(range(32)) for v in starts.values()) and len(starts) >= 7, starts
    assert longest == 2286 and any(H.header_bits(h[2]) == 2254 for h in hdrs["long"]) and min(H.header_bits(h[2]) for h in hdrs["long"]) < 2000
    assert kinds >= {"between", "plain", "16 extra", "18 extra"}, kinds
    worst = [h for h in good("sets") if "worst_second_level" in h[0]]
    assert len(worst) >= 12
    for name, prog, h, ok in worst:
        lit = T.spelled_lengths(h)[0]
        used = {t if isinstance(t, int) else T._LSYM[t[0]][0] for t in prog[-1][1]} | {256}
        assert H.sub_entries(lit, 8) == 404 and used >= {s for s in range(286) if lit[s] > 8} and used >= {0, 255, 256, 285}, name
    assert {h[2]["hlit"] for h in good("sets")} == set(range(30)) and {h[2]["hdist"] for h in good("sets")} == set(range(30))
    for which in ("lit", "dist"):
        got = {max(T.spelled_lengths(h[2])[which == "dist"]) for h in good("sets") if "/%s_longest" % which in h[0]}
        assert got == set(range(1, 16)), (which, got)
    assert {h[2]["hlit"] for h in hdrs["sets"] if not h[3]} >= {30, 31} and {h[2]["hdist"] for h in hdrs["sets"] if not h[3]} >= {30, 31}


def _check(fn, tag, name, z, data, want, it):
    st, used, out, crc = _run(fn, z, (len(data) + it % 3) if data is not None else CAP, mis=it % 4, omis=(it // 4) % 4)
    assert st == want, (tag, name, st, want)
    if data is not None:
        assert used == len(z) and crc == zlib.crc32(data) and out == data, (tag, name, used, len(z), len(out), len(data))


def test_emulation_reads_every_header(emu, emu_staged):
    """Every program through emul_inflate (span path) and emul_inflate_steps (step loop alone), the input misaligned by 0 .. 3
    bytes in turn: the status of the oracle restatement for all of them, consumed input, bytes and CRC-32 for the accepted ones.
    All programs on the default build and on c_serial_cl, the serial twin of the 64-bit front end; a seeded third of them on
    the other three staged builds."""
    caps, short_, pool, serial = emu_staged
    rnd = random.Random(1)
    it = n_third = 0
    for name, prog, z, data in H.everything():
        want = 0 if data is not None else oracle.inflate_raw(z, CAP)[0]
        assert want in (0, -3, -5), (name, want)
        builds = [("default", emu), ("c_serial_cl", serial)]
        if rnd.randrange(3) == 0:
            builds += [("c_caps", caps), ("c_short", short_), ("c_pool", pool)]
            n_third += 1
        for tag, L in builds:
            _check(L.emul_inflate, tag, name, z, data, want, it)
            _check(L.emul_inflate_steps, tag + "/steps", name, z, data, want, it + 1)
        it += 1
    assert it >= 1700 and n_third >= 500, (it, n_third)


@pytest.fixture(scope="module")
def emu_stats_serial():
    L = _build_variant("stats_serial_cl", ["-DMZ_STATS", "-DMZ_CL_PARALLEL=0", "-DMZ_CHASE_SMAX=1024u"])
    L.emul_stats.restype = C.POINTER(C.c_ulonglong)
    return L


def _header_stats(L, z, data):
    """counters 16 (symbols the 64-bit front end took), 18 (its steps) and 17 (symbols of the serial loop) of one decode"""
    s = L.emul_stats()
    for i in range(32):
        s[i] = 0
    st, used, out, crc = _run(L.emul_inflate, z, len(data))
    assert (st, used, out) == (0, len(z), data)
    return int(s[16]), int(s[18]), int(s[17])


def test_headers_reach_what_they_aim_at(emu_stats, emu_stats_serial):
    """The counters of the emulation (inflate_core.h MZ_STAT) against H.front_end_model, the plain statement of which operations
    the 64-bit front end takes and in how many steps: exactly those, for every accepted program of `window` and `long` -- a
    symbol that ends exactly at bit 64 belongs to the window it ends in, the last length of the header to the front end where
    it reaches it.  Over `window` both the front end and the serial loop behind it take symbols.  A header of `long` that runs
    past the 2048-bit register window has every operation that starts behind the window read by the serial loop, from memory.
    The build without the front end counts no front-end symbol, and reads every operation serially."""
    fe = steps = serial = last = 0
    for name, prog, z, data in H.family("window"):
        if data is not None:
            h = H.header_of(prog)[1]
            want = H.front_end_model(h, H.header_bit(prog), 8 * len(z))
            assert _header_stats(emu_stats, z, data) == want, (name, want)
            fe, steps, serial = fe + want[0], steps + want[1], serial + want[2]
            last += want[2] == 0
            assert _header_stats(emu_stats_serial, z, data) == (0, 0, len(h["ops"])), name
    print("window: %d symbols in %d front-end steps, %d symbols in the serial loop, %d headers read by the front end alone" % (fe, steps, serial, last))
    assert fe > 0 and steps > 0 and serial > 0 and last >= 60
    past = 0
    for name, prog, z, data in H.family("long"):
        k, h = H.header_of(prog)
        edge, at, behind = _aligned_edge(prog), H.ops_start(h), 0
        for op in h["ops"]:
            behind += at >= edge
            at += H.op_bits(h, op)
        want = H.front_end_model(h, H.header_bit(prog), 8 * len(z))
        assert _header_stats(emu_stats, z, data) == want, (name, want)
        if at > edge:
            past += 1
            assert want[2] > 0 and want[2] >= behind and want[0] > 0, (name, want, behind)
        assert _header_stats(emu_stats_serial, z, data) == (0, 0, len(h["ops"])), name
    assert past >= 100, past


def test_many_wave_window_on_the_mock():
    """Programs of 4 to 40 dynamic blocks, every block with another accepted header program of clc, ops, window and sets and 300
    bits of tokens or more, through the host mock's mzhip_inflate_parallel_host (inflate_parallel.inc over the emulated device
    functions: k_inflate_blocks' instantiation of mz_block_code), with the assertions of T.run_window_program."""
    if os.path.isdir("/root/reference"):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True, capture_output=True)
    if not os.path.exists(MOCK):
        pytest.skip("tests/emul/_build/libmockdrop.so needs the reference sources at build time")
    L = C.CDLL(MOCK)
    progs = H.window_programs()
    nblk = 0
    seen = set()
    for name, prog, hist in progs:
        assert 4 <= len(prog) <= 40 and all(b[0] == "dynamic" for b in prog), name
        seen |= {id(b[3]["hdr"]) for b in prog}
        b, n = T.run_window_program(L, name, prog, hist)
        nblk += b
    print("many-wave window on the mock: %d programs, %d different headers, %d blocks decoded by waves of their own" % (len(progs), len(seen), nblk))
    assert len(seen) == sum(len(p[1]) for p in progs) and nblk >= len(seen) - 2 * len(progs)
