"""CPU tests of the LZMA packet walker (tests/lzma_tokens.py) and, with it, of what K6 promises about the STRUCTURE of its
output, on the 64-lane host emulation.

First the walker is held against two judges it shares nothing with: the packet programs of tests/lzma_packets.py (streams
written packet by packet, liblzma their judge) must come back packet for packet, their refused twins must raise at or before
the packet the programs name, and liblzma's own .lzma and .xz output must walk to its input.  Only then is the walker used as
the judge of K6: emul_lzma_encode_ways at both parse classes and emul_lzma2_chunks_encode over synth.lzma_echo_cases --
reach (the echo at history_bytes() - 1 taken, the one at history_bytes() not), seams, header, end marker, chunk framing.
tests/test_gpu_lzma_tokens.py asserts the same on the device and holds the device's bytes against this emulation's."""
import ctypes as C
import lzma as pylzma
import os
import time
import zlib

import numpy as np
import pytest

from tests import lzma_packets as K
from tests import lzma_tokens as T
from tests import synth
from tests.test_kernel_emul import _build_variant, _u8p


def rows_of(packets):
    """the rows the walker must return for a list of lzma_packets packets: literal runs collapsed, positions by the lengths"""
    rows, pos, run = [], 0, False
    for p in packets:
        k = p[0]
        if k == "lit":
            if run:
                rows[-1][2] += 1
            else:
                rows.append([pos, T.LITERALS, 1, 0])
            run = True
            pos += 1
            continue
        run = False
        if k == "match":
            rows.append([pos, T.MATCH, p[2], p[1]])
            pos += p[2]
        elif k == "rep":
            rows.append([pos, T.REP0 + p[1], p[2], None])         # (the distance is whatever the queue holds)
            pos += p[2]
        elif k == "shortrep":
            rows.append([pos, T.SHORTREP, 1, None])
            pos += 1
        else:
            rows.append([pos, T.EOS, p[1], 1 << 32])
    return rows


def _same_rows(got, want, name):
    assert len(got) == len(want), (name, len(got), len(want))
    w = np.array([[r[0], r[1], r[2], -1 if r[3] is None else r[3]] for r in want], dtype=np.int64).reshape(-1, 4)
    known = w[:, 3] >= 0
    bad = np.flatnonzero((got[:, :3] != w[:, :3]).any(axis=1) | (known & (got[:, 3] != w[:, 3])))
    assert bad.size == 0, (name, "packet %d: walked %s, written %s" % (bad[0], got[bad[0]].tolist(), w[bad[0]].tolist()))


def test_walker_returns_the_packet_programs():
    """every accepted method-14 program: exactly the packets it was written from (kinds, lengths, distances; a rep's distance
    is the queue's, checked through the bytes), the bytes of expand(), one end marker, code 0, every byte used"""
    n = npk = 0
    for p, want in K.accepted() + [(q, bytes(q.expand()[0])) for q in K.big_programs()]:
        wk, head = T.walk_zip14(p.zip14(), liblzma=True)
        assert (head["lc"], head["lp"], head["pb"], head["dict_size"]) == (p.lc, p.lp, p.pb, p.dict_size), p.name
        assert wk.data == want and wk.eos and wk.code == 0 and 9 + wk.used == len(p.zip14()), p.name
        _same_rows(wk.packets, rows_of(p.packets), p.name)
        n += 1
        npk += len(wk.packets)
    print("%d programs, %d packets walked" % (n, npk))
    assert n >= 150


def test_walker_refuses_what_the_programs_name():
    """every refused program raises LzmaError -- a packet the format forbids at, or before, the output position of the packet
    expand() names; a header, a first coder byte or a last coder word the format forbids anywhere"""
    n = 0
    for p in K.refused():
        want, verdict = p.expand()
        with pytest.raises(T.LzmaError) as e:
            T.walk_zip14(p.zip14(), liblzma=True)
        if isinstance(p.note["refused"], int):
            assert verdict == ("refused", p.note["refused"]), p.name
            assert e.value.out_pos is not None and e.value.out_pos <= len(want), (p.name, str(e.value), len(want))
        n += 1
    assert n >= 100
    # a distance that liblzma's rounded dictionary accepts and the header's own figure does not: refused under the plain rule
    p = next(q for q, _ in K.accepted() if q.name == "dictionary/4097/at/match")
    with pytest.raises(T.LzmaError, match="beyond the dictionary"):
        T.walk_zip14(p.zip14())
    z = K.Program("tail", [("lit", 1), ("eos", 2)]).zip14()
    with pytest.raises(T.LzmaError, match="data behind the end"):
        T.walk_zip14(z + b"\x00")
    with pytest.raises(T.LzmaError, match="input ends"):
        T.walk_zip14(z[:-1])


def test_walker_returns_the_chunk_programs():
    """LZMA2: every accepted chunk program comes back chunk for chunk (control, sizes, properties, stored or not) and packet
    for packet with expand()'s bytes; every refused one raises"""
    n_ok = n_bad = 0
    for p in K.chunk_programs():
        want, verdict = p.expand()
        want = bytes(want)
        raw = p.raw()
        if not (verdict is None or verdict[0] == "end"):
            with pytest.raises(T.LzmaError):
                T.walk_lzma2(raw, p.dict_size, liblzma=True)
            n_bad += 1
            continue
        w2 = T.walk_lzma2(raw, p.dict_size, liblzma=True)
        assert w2.data == want, p.name
        chunks = p.chunks[:verdict[1]] if verdict else p.chunks
        assert len(w2.chunks) == len(chunks), (p.name, len(w2.chunks), len(chunks))
        rows, off = [], 0
        for ch, c in zip(chunks, w2.chunks):
            assert c.out_start == off and bool(c.stored) == (ch[0] == "raw") and (c.control & 0xE0 if not c.stored else c.control) == (ch[1] & 0xE0 if ch[0] != "raw" else ch[1]), (p.name, c)
            if ch[0] == "raw":
                assert c.usize == c.csize == len(ch[2]) and c.npackets == 0, (p.name, c)
            else:
                mine = rows_of(ch[2])
                assert c.first_packet == len(rows) and c.npackets == len(mine) and c.code == 0, (p.name, c)
                rows += [[r[0] + off] + r[1:] for r in mine]
            off += c.usize
        _same_rows(w2.packets, rows, p.name)
        x = p.xz(1)
        xw = T.walk_xz(x, liblzma=True)
        assert xw.data == want and xw.used == len(x) and len(xw.blocks) == 1, p.name
        n_ok += 1
    print("chunk programs: %d walked, %d refused" % (n_ok, n_bad))
    assert n_ok >= 250 and n_bad >= 300


def test_walker_reads_liblzma():
    """liblzma's own output walks to its input: .lzma and .xz at presets 0, 6 and 9 over the data of synth.xz_cases(), and the
    ready-made .xz streams of those cases that have LZMA2 as their only filter (every check type, stored chunks, several
    chunks, several blocks).  The measured speed is printed."""
    datas = {}
    for name, d, x in synth.xz_cases():
        datas.setdefault(name.split("/")[0], d)
    nbytes, t0 = 0, time.time()
    for name, d in sorted(datas.items()):
        for preset in (0, 6, 9):
            wk = T.walk_alone(pylzma.compress(d, format=pylzma.FORMAT_ALONE, preset=preset))
            assert wk.data == d and wk.eos and wk.code == 0, (name, preset)
            x = pylzma.compress(d, format=pylzma.FORMAT_XZ, preset=preset)
            xw = T.walk_xz(x, liblzma=True)
            assert xw.data == d and xw.used == len(x), (name, preset)
            nbytes += 2 * len(d)
    dt = time.time() - t0
    print("walked %.1f MB of liblzma output in %.2f s (compression included)" % (nbytes / 1e6, dt))
    n = 0
    for name, d, x in synth.xz_cases():
        try:
            xw = T.walk_xz(x, liblzma=True)
        except T.LzmaError as e:
            assert "reads LZMA2 alone" in str(e), (name, str(e))      # (Delta / BCJ chains: not this walker's business)
            continue
        assert xw.data == d, name
        n += 1
    assert n >= 40
    with pytest.raises(T.LzmaError, match="behind the stream footer"):
        T.walk_xz(synth.xz_cases()[0][2] + b"\x00\x00\x00\x00")


# ---- K6 on the emulation ----------------------------------------------------------------------------------------------------
_EMU = {}


def emul():
    """the emulation of tests/test_kernel_emul.py (its build knobs, MZ_EMUL_DEFS, included), optimised: the far cases are 8.4 MB"""
    if "L" not in _EMU:
        L = _build_variant("lzenc", ["-O2"] + os.environ.get("MZ_EMUL_DEFS", "").split())
        L.emul_lzma_encode_ways.argtypes = [_u8p, C.c_uint32, C.c_uint32, C.c_uint32, _u8p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.emul_lzma2_chunks_encode.argtypes = [_u8p, C.c_uint32, C.c_uint32, _u8p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.emul_set_far_depth.argtypes = [C.c_uint32]
        L.emul_lzma_encode_history_bytes.restype = C.c_uint32
        _EMU["L"] = L
    return _EMU["L"]


def depth_for_preset(preset):
    """lzma_enc_core.h MZ_LZE_DEPTH_FOR_PRESET"""
    return 1 if 0 <= preset <= 3 else 4 if preset in (4, 5) else 16 if preset >= 7 else 8


def emul_encode(d, ways, depth=0):
    """-> K6's method-14 payload for d from the emulation (depth 0: the class's default)"""
    L = emul()
    a = np.frombuffer(d, dtype=np.uint8).copy() if d else np.zeros(1, np.uint8)
    out = np.zeros(len(d) + len(d) // 8 + 1024, np.uint8)
    ol, crc = C.c_uint32(), C.c_uint32()
    L.emul_set_far_depth(depth)
    try:
        st = L.emul_lzma_encode_ways(C.cast(a.ctypes.data, _u8p), len(d), 0, ways, C.cast(out.ctypes.data, _u8p), len(out), C.byref(ol), C.byref(crc))
    finally:
        L.emul_set_far_depth(0)
    assert st == 0 and crc.value == zlib.crc32(d), (st, len(d))
    return out[:ol.value].tobytes()


def emul_xz(d, ways, depth=0):
    """-> the .xz stream mzhip_xz_encode_host lays out around the emulation's chunk payloads (as test_lzma_encode_roundtrip
    frames them: a chunk that did not shrink, or did not fit its room, is stored)"""
    L = emul()
    nch = (len(d) + 65535) // 65536
    stride = 65536 + 8192 + 1024
    a = np.frombuffer(d, dtype=np.uint8).copy() if d else np.zeros(1, np.uint8)
    outb = np.zeros(max(nch, 1) * stride, dtype=np.uint8)
    lens = (C.c_uint32 * max(nch, 1))()
    L.emul_set_far_depth(depth)
    try:
        st = L.emul_lzma2_chunks_encode(C.cast(a.ctypes.data, _u8p), len(d), ways, C.cast(outb.ctypes.data, _u8p), stride, lens)
    finally:
        L.emul_set_far_depth(0)
    assert st in (0, -200), st
    body = b""
    for i in range(nch):
        piece = d[i * 65536:(i + 1) * 65536]
        zc = outb[i * stride:i * stride + lens[i]].tobytes()
        us, cs = len(piece), len(zc)
        if cs >= us or cs > 65536 or (st != 0 and cs + 16 >= stride):
            body += bytes([1 if i == 0 else 2, (us - 1) >> 8, (us - 1) & 255]) + piece
        else:
            body += bytes([(0xE0 if i == 0 else 0xC0) | ((us - 1) >> 16), ((us - 1) >> 8) & 255, (us - 1) & 255, (cs - 1) >> 8, (cs - 1) & 255, 0x5D]) + zc
    body += b"\x00"
    flags = b"\x00\x01"
    bh = bytes([2, 0, 0x21, 1, 0x16 if nch > 1 else 8, 0, 0, 0])
    x = b"\xfd7zXZ\x00" + flags + zlib.crc32(flags).to_bytes(4, "little") + bh + zlib.crc32(bh).to_bytes(4, "little")
    x += body + b"\x00" * (-len(body) % 4) + zlib.crc32(d).to_bytes(4, "little")
    idx = b"\x00\x01" + synth._vli(12 + len(body) + 4) + synth._vli(len(d))
    idx += b"\x00" * (-len(idx) % 4)
    idx += zlib.crc32(idx).to_bytes(4, "little")
    tail = (len(idx) // 4 - 1).to_bytes(4, "little") + flags
    return x + idx + zlib.crc32(tail).to_bytes(4, "little") + tail + b"YZ"


def far_bytes():
    return int(emul().emul_lzma_encode_history_bytes())


def is_far_sized(name, far):
    return name in ("far/%d" % d for d in (far - 1, far, far + 1))


def _twin_cases(ways):
    far = far_bytes()
    return [c for c in synth.lzma_echo_cases(far) if ways > 1 or not is_far_sized(c[0], far)]


@pytest.mark.parametrize("ways", (1, 4), ids=("one-way", "four-way"))
def test_emul_method14_packets(ways):
    """emul_lzma_encode_ways over every case of synth.lzma_echo_cases (the far-sized ones at the four-way class only):
    lzma_tokens.check_encoded, and liblzma reads every stream."""
    far = far_bytes()
    for name, d, period in _twin_cases(ways):
        z = emul_encode(d, ways)
        T.check_encoded(z, d, ways == 1, far, where=(name,), period=period, near_cover=name in ("near/32767", "near/32768"))
        assert pylzma.decompress(z[4:9] + b"\xff" * 8 + z[9:], format=pylzma.FORMAT_ALONE) == d, name


@pytest.mark.parametrize("ways", (1, 4), ids=("one-way", "four-way"))
def test_emul_xz_chunks(ways):
    """emul_lzma2_chunks_encode over the same cases, framed as mzhip_xz_encode_host frames them: lzma_tokens.check_xz -- the
    chunk rules, the packet rules with positions counted over the block (a far echo across chunks is used), and the block of
    noise in front of text stored (0x01) with the text behind it coded (0xC0)."""
    far = far_bytes()
    for name, d, period in _twin_cases(ways):
        x = emul_xz(d, ways)
        xw = T.check_xz(x, d, far, where=(name, "%d-way" % ways), period=period, near_cover=name in ("near/32767", "near/32768"))
        if name == "noise+text":
            assert [c.control for c in xw.blocks[0].walk.chunks] == [0x01, 0xC0], name
