"""CPU tests of the packet programs (tests/lzma_packets.py): LZMA1 / LZMA2 streams written packet by packet.

First the writer is held against the judge: every accepted program decodes under liblzma (Python's lzma) to what expand()
says, every refused twin raises there, and the oracle restatement agrees with liblzma.  Then every program goes through the
host emulation of the device cores -- the full-model build, the slot build (MZHIP_RETRY or the same result), the .xz kernel
and the two resumable builds, window by window -- and counters that exist in the emulation only (lzma_core.h LZ_STAT) hold
each family to what it is named for."""
import ctypes as C
import lzma as pylzma
import zlib

import pytest

import oracle
from tests import lzma_packets as K
from tests.test_kernel_emul import _build_variant, _lzma2_windows, _lzma_windows, _run, _u8p

CHECKS = (0, 1, 4, 10)           # the check types the .xz kernel verifies: none, CRC-32, CRC-64, SHA-256
NSTAT = 32


@pytest.fixture(scope="module")
def emu():
    L = _build_variant("lzstats", ["-DMZ_LZ_STATS"])
    L.emul_lzma.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32, C.c_int64] + [C.POINTER(C.c_uint32)] * 3
    L.emul_lzma_slots.argtypes = L.emul_lzma.argtypes
    L.emul_xz.argtypes = L.emul_lzma.argtypes
    L.emul_lzma_resume.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.emul_lz_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    L.emul_lz_stats.restype = None
    return L


def _stats(emu, reset=True):
    a = (C.c_uint64 * NSTAT)()
    emu.emul_lz_stats(a, 1 if reset else 0)
    return list(a)


def _liblzma_alone(z):
    """-> (bytes or None, "ok" | "cut" | "refused", unused bytes)"""
    d = pylzma.LZMADecompressor(format=pylzma.FORMAT_ALONE)
    try:
        got = d.decompress(z)
    except pylzma.LZMAError:
        return None, "refused", 0
    return got, ("ok" if d.eof else "cut"), len(d.unused_data)


def _liblzma_raw2(z, dict_size):
    d = pylzma.LZMADecompressor(format=pylzma.FORMAT_RAW, filters=[dict(id=pylzma.FILTER_LZMA2, dict_size=max(dict_size, 4096))])
    try:
        got = d.decompress(z)
    except pylzma.LZMAError:
        return None, "refused", 0
    return got, ("ok" if d.eof else "cut"), len(d.unused_data)


# ---- the writer against the judge ----------------------------------------------------------------------------------------
def test_writer_against_liblzma():
    """method 14: every accepted program decodes under liblzma (FORMAT_ALONE, unknown size) to expand(), with no byte left
    over; every refused twin raises; the oracle restatement gives status 0 / -3, the consumed count and the bytes liblzma
    gives."""
    n_ok = n_bad = nbytes = 0
    per = {}
    for p in K.all_programs() + K.big_programs() + [c[0] for c in K.out_cap_cases()]:
        want, verdict = p.expand()
        got, how, unused = _liblzma_alone(p.alone())
        z = p.zip14()
        so, uo, oo = oracle.lzma_zip_decode(z, len(want) + 300, -1)
        fam = p.name.split("/")[0]
        per[fam] = per.get(fam, 0) + 1
        if "refused" in p.note:
            assert how == "refused", (p.name, how)
            assert so == -3, (p.name, so)
            if isinstance(p.note["refused"], int):
                assert verdict == ("refused", p.note["refused"]), (p.name, verdict)
            assert bytes(want).startswith(oo[:len(want)]) or oo.startswith(bytes(want)), p.name
            n_bad += 1
        else:
            assert verdict == "end" and how == "ok" and unused == 0 and got == bytes(want), (p.name, verdict, how, unused)
            assert (so, uo, oo) == (0, len(z), got), (p.name, so, uo, len(z))
            n_ok += 1
            nbytes += len(got)
    print("packet programs per family: %s; %d accepted, %d refused, %d bytes of output" % (per, n_ok, n_bad, nbytes))
    assert n_ok >= 150 and n_bad >= 100
    if oracle.have_ref():
        ref = oracle.ref()
        for p, want in K.accepted():
            z = p.zip14()
            r = ref.stream_decode(14, z, len(want) + 8, max_in=len(z), max_out=len(want))
            assert r["out"] == want and r["error"] == 0, p.name
        for p in K.refused():
            r = ref.stream_decode(14, p.zip14(), 400000, max_in=len(p.zip14()))
            assert r["error"] != 0, p.name


def test_chunk_writer_against_liblzma():
    """LZMA2: every chunk program under FORMAT_RAW with FILTER_LZMA2 -- accepted ones give expand(), refused ones raise (or,
    cut short, never reach the end); framed into a one-block .xz with each check type they decode under FORMAT_XZ; the
    oracle restatement agrees on status, consumed bytes and bytes."""
    n_ok = n_bad = nbytes = 0
    for i, p in enumerate(K.chunk_programs()):
        want, verdict = p.expand()
        want = bytes(want)
        got, how, unused = _liblzma_raw2(p.raw(), p.dict_size)
        x = p.xz(CHECKS[i % 4])
        so, uo, oo = oracle.xz_decode(x + b"tail", len(want) + 300)
        if verdict is None or verdict[0] == "end":
            assert how == "ok" and got == want and unused == 0, (p.name, how, unused)
            assert pylzma.decompress(x, format=pylzma.FORMAT_XZ) == want, p.name
            assert (so, uo, oo) == (0, len(x), want), (p.name, so, uo, len(x))
            n_ok += 1
            nbytes += len(want)
        else:
            assert how != "ok", (p.name, verdict)
            assert so == -3, (p.name, verdict, so)
            with pytest.raises(pylzma.LZMAError):
                pylzma.decompress(x, format=pylzma.FORMAT_XZ)
            n_bad += 1
        if oracle.have_ref() and len(want) <= 300000:
            r = oracle.ref().stream_decode(95, x, len(want) + 300, max_in=len(x))
            if verdict is None or verdict[0] == "end":
                assert r["out"] == want and r["error"] == 0, p.name
            else:
                assert r["error"] != 0 and want.startswith(r["out"][:len(want)]), p.name
    print("chunk programs: %d accepted, %d refused, %d bytes of output" % (n_ok, n_bad, nbytes))
    assert n_ok >= 250 and n_bad >= 300


# ---- the emulation -----------------------------------------------------------------------------------------------------
WINDOWS = ((300, 65), (4096, 700), (1000, 1 << 30))      # (output window, input gulp): 65 = one byte beyond the margin


def _emul14(emu, p, want, cap_extra=5):
    """one accepted program through the full-model build, the slot build and the resumable build"""
    z = p.zip14()
    cap = len(want) + cap_extra
    a = _run(emu.emul_lzma, z, cap, C.c_int64(-1), mis=len(z) & 3, omis=len(want) & 3)
    assert a == (0, len(z), want, zlib.crc32(want)), (p.name, a[0], a[1], len(z), len(a[2]), len(want))
    b = _run(emu.emul_lzma_slots, z, cap, C.c_int64(-1))
    assert b[0] == -300 or b == a, (p.name, b[0])
    return b[0] == -300


def test_emulation_lzma1(emu):
    """every accepted method-14 program: status 0, out_len, in_used == len(stream), bytes, CRC-32 -- out_cap exact for every
    second one; every refused twin: the oracle's status, nothing written beyond out_cap (the red zones of _run)"""
    _stats(emu)
    back = 0
    for i, (p, want) in enumerate(K.accepted()):
        back += _emul14(emu, p, want, cap_extra=0 if i % 2 else 7)
    for p in K.refused():
        z = p.zip14()
        cap = len(p.expand()[0]) + 50
        so = oracle.lzma_zip_decode(z, cap, -1)[0]
        a = _run(emu.emul_lzma, z, cap, C.c_int64(-1))
        b = _run(emu.emul_lzma_slots, z, cap, C.c_int64(-1))
        assert a[0] == so == -3 and b[0] in (so, -300), (p.name, a[0], b[0], so)
        want = bytes(p.expand()[0])
        assert want.startswith(a[2]) and want.startswith(b[2]), (p.name, len(a[2]), len(b[2]), len(want))
    st = _stats(emu)
    print("emulation, method 14: %d accepted, %d given back by the slot build, %d refused; counters %s" % (len(K.accepted()), back, len(K.refused()), st))


def test_emulation_big_entries(emu):
    """the named entries above 256 KiB: distance-1 runs of 1, 2 and 4 MiB with distances up to slot 43 behind them"""
    for p in K.big_programs():
        want = bytes(p.expand()[0])
        _emul14(emu, p, want)
        assert p.note["top"] >= 39


def test_emulation_windows(emu):
    """the resumable build, window by window (the drivers of test_kernel_emul.py): every accepted program in windows of 300
    bytes from gulps of 65 input bytes -- one byte more than the margin in front of a packet -- and two wider forms"""
    _stats(emu)
    n = 0
    for i, (p, want) in enumerate(K.accepted()):
        z = p.zip14()
        for window, gulp in (WINDOWS if len(want) < 60000 or p.name.startswith("expensive") else WINDOWS[1:2]):
            got, used, rc = _lzma_windows(emu, z, len(want), window, gulp, K.round_dict(p.dict_size))
            assert (rc, used) == (0, len(z)) and got == want, (p.name, window, gulp, rc, used, len(z), len(got), len(want))
            n += 1
    st = _stats(emu)
    print("resumable build: %d walks, %d stops in front of a packet" % (n, st[22]))
    assert st[22] > 10000
    for p in K.refused()[::3]:
        z = p.zip14()
        got, used, rc = _lzma_windows(emu, z, 0, 4096, 700, K.round_dict(p.dict_size))
        assert rc == -3, (p.name, rc)


def test_family_states(emu):
    """every edge of the state graph is coded at every pos_state of every pb (the writer's own count of (state, kind,
    pos_state) triples); the decoder sees matched literals leave the match tree at each of the 8 bit positions and never"""
    for p in K.family("states"):
        c = p.encode()[1]
        want = bytes(p.expand()[0])
        _stats(emu)
        _emul14(emu, p, want)
        st = _stats(emu)
        if p.note.get("edges"):
            kinds = set(c.stats["kinds"])
            want_kinds = {(s, kind, ps) for s in range(12) for kind in ("lit", "match", "rep0", "rep1", "rep2", "rep3", "shortrep")
                          for ps in range(1 << p.pb)}
            assert not want_kinds - kinds, (p.name, sorted(want_kinds - kinds)[:10])
        if p.note.get("leave"):
            assert all(c.stats["leave"][k] >= 8 for k in range(9)), (p.name, c.stats["leave"])
            # the slot build ran as well: twice the writer's count unless it gave the entry back
            assert all(st[5 + k] >= c.stats["leave"][k] for k in range(9)), (p.name, st[5:14], c.stats["leave"])


def test_family_literals(emu):
    """lc + lp = 4: plain and matched literals in both halves of the model -- the upper half through LZ_BIT_X"""
    seen = 0
    for p in K.family("literals"):
        if "refused" in p.note:
            continue
        want = bytes(p.expand()[0])
        _stats(emu)
        z = p.zip14()
        a = _run(emu.emul_lzma, z, len(want), C.c_int64(-1))
        assert a == (0, len(z), want, zlib.crc32(want)), p.name
        st = _stats(emu)
        c = p.encode()[1]
        assert sum(st[5:14]) == sum(c.stats["leave"]) > 20, p.name
        if p.lc + p.lp == 4:
            seen += 1
            assert st[2] > 0 and st[3] > 0 and st[4] > 0, (p.name, st[:5])          # upper half: both literal forms
            assert sum(st[5:14]) > st[3] and len(want) > st[3] + st[4], p.name          # ... and the lower half as well
        else:
            assert st[2] == 0
    assert seen == 5


def test_family_slots(emu):
    """K3's slot build on programs that control its swaps: which are given back (MZHIP_RETRY), after how many swaps and at
    which output position -- as predict_slots restates the rule 64 + (opos >> 7) -- and that the full-model build then
    decodes them"""
    for p in K.family("slots"):
        want = bytes(p.expand()[0])
        z = p.zip14()
        _stats(emu)
        b = _run(emu.emul_lzma_slots, z, len(want), C.c_int64(-1))
        st = _stats(emu)
        gave, swaps, at = K.predict_slots(p)
        print("%s: %d bytes, %d swaps, %s" % (p.name, len(want), st[0], "given back at output position %d" % st[23] if st[1] else "kept"))
        assert (b[0] == -300) == gave == bool(st[1]) and st[0] == swaps, (p.name, b[0], gave, st[0], swaps)
        if gave:
            assert st[23] == at and len(b[2]) == at, (p.name, st[23], at)
        else:
            assert b == (0, len(z), want, zlib.crc32(want)), p.name
        a = _run(emu.emul_lzma, z, len(want), C.c_int64(-1))
        assert a == (0, len(z), want, zlib.crc32(want)), p.name
        if "back" in p.note and p.note["back"] is not None:
            assert gave == p.note["back"], p.name
        if p.note.get("swaps"):
            assert swaps == p.note["swaps"], (p.name, swaps)
        if "back_at" in p.note:
            assert at == p.note["back_at"]
        if p.note.get("late"):
            assert 0.9 * p.note["late"] <= at <= 1.1 * p.note["late"] + 400, (p.name, at, p.note["late"])


def test_family_window(emu):
    """compressed lengths 9 + 256 k + r: the refill count is k (k - 1 where the last window ends with the stream); code != 0
    behind the marker and a non-zero first byte are refused; every prefix of three short programs gives what liblzma gives"""
    lens = set()
    for p in K.family("window"):
        if "refused" in p.note:
            continue
        z = p.zip14()
        want = bytes(p.expand()[0])
        _stats(emu)
        a = _run(emu.emul_lzma, z, len(want), C.c_int64(-1))
        st = _stats(emu)
        assert a == (0, len(z), want, zlib.crc32(want)), p.name
        assert st[14] == (len(z) - 9 - 1) // 256, (p.name, len(z), st[14])
        lens.add(len(z) - 9)
    assert lens == {256 * k + r for k in range(4) for r in (0, 1, 2, 3, 4, 255) if 256 * k + r >= 6}, sorted(lens)
    cut = ref = 0
    for p in K.prefix_programs():
        z = p.zip14()
        want = bytes(p.expand()[0])
        assert len(z) - 9 <= 300
        for n in range(len(z)):
            got, how, _ = _liblzma_alone(p.alone()[:n + 4]) if n >= 9 else (b"", "cut", 0)
            so, uo, oo = oracle.lzma_zip_decode(z[:n], len(want) + 10, -1)
            a = _run(emu.emul_lzma, z[:n], len(want) + 10, C.c_int64(-1), mis=n & 3)
            b = _run(emu.emul_lzma_slots, z[:n], len(want) + 10, C.c_int64(-1))
            assert how != "ok" and so != 0
            assert a[0] in (-3, -5) and (a[0] == -5) == (how == "cut"), (p.name, n, a[0], how)
            assert want.startswith(a[2]) and (b[0] == -300 or b[:3] == a[:3]), (p.name, n)
            if how == "cut":
                assert a[2] == got[:len(a[2])] and len(got) - len(a[2]) <= 273 + 1, (p.name, n, len(got), len(a[2]))
            cut += how == "cut"
            ref += how == "refused"
    print("prefixes: %d truncated, %d refused" % (cut, ref))
    assert cut > 500


def test_family_overlap_caps(emu):
    """copies that end exactly at out_cap, that are cut there (-200, the bytes up to the cap written and nothing behind), a
    literal and a short rep at out_cap"""
    _stats(emu)
    for p, cap, status, out_len in K.out_cap_cases():
        z = p.zip14()
        want = bytes(p.expand()[0])
        so, uo, oo = oracle.lzma_zip_decode(z, cap, -1)
        for fn in (emu.emul_lzma, emu.emul_lzma_slots):
            a = _run(fn, z, cap, C.c_int64(-1), omis=cap & 3)
            assert a[0] == status == so and a[2] == want[:out_len] == oo, (p.name, a[0], status, so, len(a[2]), out_len)
    assert _stats(emu)[15] >= 12


def _walk(p):
    """(kind, distance, length, output position) of every copy of a program, from the packets alone"""
    pos, reps = 0, [0, 0, 0, 0]
    for q in p.packets:
        if q[0] == "match":
            reps = [q[1] - 1] + reps[:3]
            yield "match", q[1], q[2], pos
            pos += q[2]
        elif q[0] == "rep":
            reps.insert(0, reps.pop(q[1]))
            yield "rep", reps[0] + 1, q[2], pos
            pos += q[2]
        elif q[0] != "eos":
            pos += 1


def test_family_lengths(emu):
    """every length 2 .. 273 through the match and the rep length coder at every pos_state of pb 0, 2 and 4 (the writer's own
    count of (coder, length, pos_state)); the programs decode"""
    for pb in (0, 2, 4):
        seen = set()
        for p in K.family("lengths"):
            if p.pb == pb:
                seen |= p.encode()[1].stats["lens"]
        want = {(c, n, ps) for c in ("match", "rep") for n in range(2, 274) for ps in range(1 << pb)}
        assert not want - seen, (pb, sorted(want - seen)[:10])
    assert {p.packets[-1][1] for p in K.family("lengths")} >= {273 - n % 7 for n in (273,)}       # an end marker behind a long length


def test_family_distances(emu):
    """slots 0 .. 35 (35: its low distances) in all four len-to-slot-tree classes with low, high and random footer bits -- the reverse trees of slots
    4 .. 13, direct bits and align from 14 on --, refused twins for every slot from 36 on"""
    p = K.family("distances")[0]
    seen = p.encode()[1].stats["slots"]
    want = {(cls, slot) for cls in range(4) for slot in range(36)}
    assert p.note["slots"] == list(range(36)) and not want - seen, sorted(want - seen)[:10]
    dists = {}
    for kind, d, n, pos in _walk(p):
        if pos > K.SLOT_CAP - 300:
            dists.setdefault(max(d - 1, 1).bit_length(), set()).add(d - 1)
    for nb in range(3, 18):               # distances of nb bits: the lowest and the highest of both slots
        assert {1 << (nb - 1), (3 << (nb - 2)) - 1, 3 << (nb - 2), (1 << nb) - 1} <= dists[nb], nb
    bad = {int(q.name.split("/")[2][4:]) for q in K.family("distances") if "refused" in q.note}
    assert bad >= set(range(36, 64)), sorted(set(range(36, 64)) - bad)
    tops = [q.note["top"] for q in K.big_programs()]
    assert max(tops) == 43                 # the runs of 1, 2 and 4 MiB reach the valid distances of slots up to 43


def test_family_reps(emu):
    """the rep queue under every sequence of three reps behind four fresh distances (64 of them), reps before a distance was
    set, and a rep / short rep at position 0 refused at packet 0"""
    progs = {p.name: p for p in K.family("reps")}
    q = progs["reps/queue"]
    triples, cur = set(), None
    for pk in q.packets:
        if pk == ("match", 5, 2):
            cur = []
        elif pk[0] == "rep" and cur is not None:
            cur.append(pk[1])
            if len(cur) == 3:
                triples.add(tuple(cur))
    assert len(triples) == 64
    kinds = q.encode()[1].stats["kinds"]
    assert all(sum(v for (s, k, ps), v in kinds.items() if k == "rep%d" % i) >= 48 for i in range(4))
    for k in range(4):
        assert progs["reps/unset/rep%d" % k].expand()[1] == "end"
        assert progs["reps/refused/pos0/rep%d" % k].expand()[1] == ("refused", 0)
    assert progs["reps/refused/pos0/shortrep"].expand()[1] == ("refused", 0)


def test_family_dictionary(emu):
    """for every header dictionary size: the distance at the rounded size, one below and one above, as a match, as rep0 .. 3
    and as a short rep -- `above` refused at the match that sets it, the others accepted and decoded"""
    progs = {p.name: p for p in K.family("dictionary")}
    assert len(progs) == len(K.DICT_SIZES) * 3 * 6
    for ds in K.DICT_SIZES:
        lim = K.round_dict(ds)
        assert lim >= 4096 and lim % 16 == 0 and lim - 15 <= max(ds, 4096) <= lim
        for what, dist in (("at", lim), ("below", lim - 1), ("above", lim + 1)):
            for use in ("match", "rep0", "rep1", "rep2", "rep3", "shortrep"):
                p = progs["dictionary/%d/%s/%s" % (ds, what, use)]
                far = [(k, d, n, pos) for k, d, n, pos in _walk(p) if d == dist]
                assert far and far[0][0] == "match" and far[0][3] >= dist, p.name      # the output reaches: only the dictionary decides
                if what == "above":
                    assert p.expand()[1][0] == "refused" and "refused" in p.note, p.name
                else:
                    assert p.expand()[1] == "end", p.name
                    if use.startswith("rep"):
                        assert any(k == "rep" for k, d, n, pos in far), p.name
                    if use == "shortrep":
                        assert ("shortrep",) in p.packets


def test_family_overlap(emu):
    """every dist 1 .. 70 with every length of the family at every output offset mod 64"""
    seen = set()
    for p in K.family("overlap"):
        for kind, d, n, pos in _walk(p):
            if d in p.note["dists"] and (kind == "rep" or n > 2 or pos % 3):
                seen.add((d, n, pos % 64))
    lens = (63, 64, 65, 127, 128, 129, 272, 273)
    want = {(d, n, off) for d in range(1, 71) for n in lens for off in range(64)}
    assert not want - seen, sorted(want - seen)[:10]
    assert {(d, 2) for d in range(1, 71)} <= {(d, n) for d, n, off in seen}


def test_family_expensive(emu):
    """packets trained to cost as much as the model allows: the largest one, in compressed bytes, against the 64-byte margin
    of LZ_RESUME_CHECK.  The resumable build is stopped exactly in front of each of them (by the room in its output window),
    then handed 64 bytes of input and no more: it decodes the packet from them and stops behind it."""
    worst = 0
    for p in K.family("expensive"):
        pb = p.packet_bytes()
        worst = max(worst, max(pb))
        k = p.note["strike"]
        assert pb[k] >= 12 and pb[k] == max(pb), (p.name, pb[k])      # (an untrained match of this kind: 5 bytes)
        z = p.zip14()
        want = bytes(p.expand()[0])
        before = len(K.expand(p.packets[:k], p.dict_size)[0])
        n = p.packets[k][2]
        buf = (C.c_uint8 * (len(want) + 600))()
        model = (C.c_uint16 * emu.emul_lzma_model_u16())()
        st, sto = (C.c_uint32 * 16)(), (C.c_uint32 * 16)()
        ol, iu = C.c_uint32(), C.c_uint32()
        src = (C.c_uint8 * len(z)).from_buffer_copy(z)
        st[0] = 2                            # all of the input is there: only the room in the window stops this call
        rc = emu.emul_lzma_resume(src, len(z), buf, before + 273, st, sto, model, C.byref(ol), C.byref(iu))
        assert (rc, sto[0], sto[10], ol.value) == (-200, 1, before, before) and bytes(buf[:before]) == want[:before], (p.name, rc, sto[10], before)
        used = iu.value
        assert used in (9 + p.encode()[2][k] - 1, 9 + p.encode()[2][k]), (p.name, used, p.encode()[2][k])
        for i in range(16):
            st[i] = sto[i]
        st[0] = 1
        src = (C.c_uint8 * 64).from_buffer_copy(z[used:used + 64])
        rc = emu.emul_lzma_resume(src, 64, buf, len(want) + 600, st, sto, model, C.byref(ol), C.byref(iu))
        assert (rc, sto[0], sto[10]) == (-5, 1, before + n) and bytes(buf[:before + n]) == want[:before + n], (p.name, rc, sto[10], before + n)
        assert pb[k] - 1 <= iu.value <= pb[k] + 1, (p.name, iu.value, pb[k])
    print("largest packet: %d compressed bytes (margin of the resumable builds: 64)" % worst)
    assert worst <= 64


def test_emulation_chunks(emu):
    """every chunk program, framed, through the .xz kernel's emulation, and raw through mz_lzma2_run window by window:
    accepted ones exact (status, lengths, bytes, CRC-32, the block's check), refused ones refused with the oracle's
    status; every control class is seen"""
    _stats(emu)
    n = 0
    for i, p in enumerate(K.chunk_programs()):
        want, verdict = p.expand()
        want = bytes(want)
        ok = verdict is None or verdict[0] == "end"
        chk = CHECKS[i % 4]
        x = p.xz(chk)
        cap = len(want) + (0 if i % 2 else 33)
        a = _run(emu.emul_xz, x + b"tail", cap, C.c_int64(-1), mis=i & 3, omis=(i >> 2) & 3)
        so = oracle.xz_decode(x + b"tail", cap)[0]
        if ok:
            assert a == (0, len(x), want, zlib.crc32(want)), (p.name, a[0], a[1], len(x), len(a[2]), len(want))
        else:
            assert a[0] == so == -3, (p.name, verdict, a[0], so)
        small = len(want) < 100000
        for window, gulp in (((300, 90), (4096, 700)) if small else ((65536, 20000),)):
            cid = 4 if chk != 1 else 1
            got, used, rc, cv, _ = _lzma2_windows(emu, p.raw(), window, gulp, p.dict_size, cid)
            if ok:
                assert (rc, used) == (0, len(p.raw())) and got == want, (p.name, window, rc, used, len(p.raw()), len(got), len(want))
                assert cv == (oracle.crc64(want) if cid == 4 else zlib.crc32(want)), p.name
            else:
                assert rc == -3 and want.startswith(got[:len(want)]), (p.name, verdict, window, rc)
            n += 1
    st = _stats(emu)
    print("chunk programs: %d window walks; chunks by control class (1, 2, 0x80, 0xA0, 0xC0, 0xE0, other): %s" % (n, st[16:22] + st[24:25]))
    assert all(v > 20 for v in st[16:22]) and st[24] > 100
