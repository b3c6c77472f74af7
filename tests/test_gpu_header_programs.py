"""GPU tests of the header programs (tests/header_programs.py): dynamic block headers spelled field by field -- every HCLEN and
code-length-code shape, every repeat count, runs that cross from the literal into the distance lengths, symbols that straddle
the 64-bit window of the front end, headers longer than the 2048-bit register window, the literal / length code that fills the
second-level table, and the refused and cut twins of all of them -- through the three instantiations of mz_block_code
(mzhip_inflate_batch, mzhip_inflate_resume_batch, mzhip_inflate_parallel_host) and through the header search and its check
(k_find_blocks, k_check_headers).  zlib's inflate is the judge of the decoders, tests/header_programs.read_header -- held
against zlib on the CPU by tests/test_header_programs.py -- the judge of k_check_headers.

Caps of this file: at most 4096 entries per launch, every stream below 2 KiB, every expected output below 4 KiB."""
import ctypes as C
import os
import random
import time
import zlib

import numpy as np
import pytest

import oracle
from tests import header_programs as H
from tests import token_programs as T

pytestmark = pytest.mark.gpu

MAX_ENTRIES, CAP, OUT_FULL = 4096, 4096, -200


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


@pytest.fixture(scope="module")
def entries():
    """[(name, stream, expected bytes or None, status)] of every program of every family -- accepted, refused and cut in a seeded
    order --, the status that of the oracle restatement; computed once, nobody changes it"""
    t0 = time.time()
    out = []
    for name, prog, z, data in H.everything():
        want = 0 if data is not None else oracle.inflate_raw(z, CAP)[0]
        assert want in (0, -3, -5), (name, want)
        out.append((name, z, data, want))
    random.Random(30).shuffle(out)
    n = {s: sum(e[3] == s for e in out) for s in (0, -3, -5)}
    print("header programs: %s, %d accepted, %d refused, %d cut; zlib runtime version %s; built in %.1f s"
          % ({f: len(H.family(f)) for f in H.ALL_FAMILIES}, n[0], n[-3], n[-5], zlib.ZLIB_RUNTIME_VERSION, time.time() - t0))
    assert n[0] >= 1200 and n[-3] >= 300 and n[-5] >= 200 and len(out) <= MAX_ENTRIES
    return out


def _caps(entries):
    return [(len(d) + (0 if i % 2 == 0 else 1 + (i * 7) % 64)) if d is not None else CAP for i, (_, _, d, _) in enumerate(entries)]


def _check_entry(gpu, what, batch, h_out, res, i, entry):
    name, z, data, want = entry
    out_len, in_used, crc, status = res
    assert status[i] == want, (what, name, int(status[i]), want)
    if data is None:
        return
    assert out_len[i] == len(data) and in_used[i] == len(z), (what, name, int(out_len[i]), len(data), int(in_used[i]), len(z))
    got = gpu.entry_bytes(batch, h_out, i, len(data))
    if got != data:
        bad = next(k for k in range(len(data)) if got[k] != data[k])
        raise AssertionError("%s: %s: byte %d of %d is %d, zlib says %d" % (what, name, bad, len(data), got[bad], data[bad]))
    assert int(crc[i]) == zlib.crc32(data), (what, name)


def test_batch_header_programs(gpu, entries):
    """Every program of every family in ONE launch of mzhip_inflate_batch, accepted, refused and cut interleaved: entries laid
    out byte by byte (align=1), packed and odd, and in another seeded order.  Accepted programs: status 0, out_len, in_used ==
    len(stream), the bytes and the CRC-32 against zlib's; the rest: the status of the oracle restatement (-3 or -5)."""
    t0 = time.time()
    caps = _caps(entries)
    order = list(range(len(entries)))
    random.Random(31).shuffle(order)
    for what, idx, layout in (("align=1", None, dict(align=1)), ("packed", None, dict(packed=True, odd=True)), ("shuffled", order, dict(align=1))):
        es = entries if idx is None else [entries[k] for k in idx]
        cs = caps if idx is None else [caps[k] for k in idx]
        batch = gpu.make_batch([e[1] for e in es], cs, **layout)
        res = gpu.run_inflate(batch)
        h_out = batch["d_out"].cpu().numpy()
        if what == "packed":
            assert {int(o) & 3 for o in batch["h_in_off"]} == {0, 1, 2, 3}          # every misalignment of the input
            assert batch["d_in"].data_ptr() % 4 == 0
        for i, e in enumerate(es):
            _check_entry(gpu, what, batch, h_out, res, i, e)
    print("test_batch_header_programs: 3 launches of %d entries, %.2f s" % (len(entries), time.time() - t0))


def test_resumable_build_header_programs(gpu, entries):
    """The same entries through mzhip_inflate_resume_batch with stop states asked for: k_inflate_batch<true>, another compile
    of mz_block_code.  Then the programs with blocks in front of their header once more block by block: flags bit 1 stops in
    front of every block header and the next launch takes the stream up from that state, so that the long headers are parsed
    from a state's hdr_bit at every bit 0 .. 31 modulo 32; the concatenated output equals zlib's."""
    import torch

    from tests.test_gpu_bounds import launch_inflate

    t0 = time.time()
    batch = gpu.make_batch([e[1] for e in entries], _caps(entries), align=1)
    R = launch_inflate(gpu, batch, stop=True)
    n = batch["n"]
    res = (gpu.result_words(R["out_len"], n).astype(np.int64), gpu.result_words(R["in_used"], n).astype(np.int64),
           gpu.result_words(R["crc"], n), gpu.result_words(R["status"], n).view(np.int32))
    h_out = batch["d_out"].cpu().numpy()
    for i, e in enumerate(entries):
        _check_entry(gpu, "resumable", batch, h_out, res, i, e)
    t1 = time.time()
    cases = [(name, z, data) for name, prog, z, data in H.family("long") if len(prog) > 1]
    assert len(cases) >= 150
    todo = list(range(len(cases)))
    got = {i: bytearray() for i in todo}
    state = {i: (0, 0, 0, 2) for i in todo}
    rounds = nblk = 0
    while todo:
        rounds += 1
        assert rounds <= 64
        hist = [state[i][2] for i in todo]
        b = gpu.make_batch([cases[i][1] for i in todo], [h + CAP for h in hist], align=1)
        h0 = np.zeros(b["d_out"].numel(), dtype=np.uint8)
        for k, i in enumerate(todo):
            o = int(b["h_out_off"][k])
            h0[o:o + hist[k]] = np.frombuffer(bytes(got[i][len(got[i]) - hist[k]:]), dtype=np.uint8)
        b["d_out"].copy_(torch.from_numpy(h0))
        rs = torch.tensor([state[i] for i in todo], dtype=torch.int64).to(torch.int32).to(b["d_in"].device)
        R = launch_inflate(gpu, b, resume=rs, stop=True)
        m = b["n"]
        out_len = gpu.result_words(R["out_len"], m).astype(np.int64)
        status = gpu.result_words(R["status"], m).view(np.int32)
        stop = gpu.result_words(R["stop"], m, 4)
        h = b["d_out"].cpu().numpy()
        nxt = []
        for k, i in enumerate(todo):
            name, z, data = cases[i]
            o = int(b["h_out_off"][k])
            assert status[k] in (0, OUT_FULL), (name, rounds, int(status[k]))
            valid = int(out_len[k]) if status[k] == 0 else int(stop[k][2])
            assert hist[k] <= valid <= hist[k] + CAP, (name, rounds, valid)
            got[i] += h[o + hist[k]:o + valid].tobytes()
            nblk += 1
            if status[k] == 0:
                assert bytes(got[i]) == data, (name, rounds)
                continue
            assert stop[k][3] & 1 and stop[k][0] == stop[k][1] > state[i][0], (name, rounds, list(stop[k]))   # in front of the next header
            state[i] = (int(stop[k][0]), int(stop[k][1]), min(len(got[i]), 32768), 3)
            nxt.append(i)
        todo = nxt
    assert nblk >= 4 * len(cases)
    print("test_resumable_build_header_programs: one launch of %d entries %.2f s; %d streams block by block, %d blocks in %d launches, %.2f s"
          % (len(entries), t1 - t0, len(cases), nblk, rounds, time.time() - t1))


def test_many_wave_header_programs(gpu):
    """Programs of 4 to 40 dynamic blocks, every block with another accepted header program and 300 bits of tokens or more,
    through mzhip_inflate_parallel_host: a wave of k_inflate_blocks per block (T.run_window_program asserts rc, bytes,
    checksums, block count and state against zlib)."""
    t0 = time.time()
    L = gpu.mz.lib()
    progs = H.window_programs()
    nblk = nhdr = 0
    for name, prog, hist in progs:
        assert 4 <= len(prog) <= 40 and all(b[0] == "dynamic" for b in prog), name
        b, n = T.run_window_program(L, name, prog, hist)
        nblk += b
        nhdr += len(prog)
    print("test_many_wave_header_programs: %d windows, %d headers, %d blocks decoded by waves of their own, %.2f s"
          % (len(progs), nhdr, nblk, time.time() - t0))
    assert nhdr >= 200 and nblk >= nhdr - 2 * len(progs)


def test_header_check_is_exact(gpu):
    """k_check_headers against read_header.  Several hundred header programs lie in one buffer at recorded bit offsets, each with
    its tokens and 24 .. 40 bytes of noise behind it: the accepted ones and every refused one whose code-length code is complete
    (the search passes those on).  For seven placements of the buffer relative to a 16-byte boundary: (a) k_find_blocks and the
    one-offset-per-lane statement of it return the same candidates, every recorded offset with HLIT, HDIST <= 29 and a complete
    code-length code among them; (b) of EVERY candidate -- the accidental ones inside token bits and noise included --
    k_check_headers keeps exactly those whose header read_header() gets past inside the buffer; stored candidates are kept."""
    t0 = time.time()
    L = gpu.mz.lib()
    L.mzhip_find_blocks_host.restype = C.c_int32
    L.mzhip_find_blocks_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    rnd = random.Random(32)
    picked = []
    for fam in H.FAMILIES:
        es = H.family(fam)
        good = [e for e in es if e[3] is not None]
        bad = [e for e in es if e[3] is None and H._kraft_left(H.header_of(e[1])[1]["cl"], 7)[0] == 0]
        picked += rnd.sample(good, min(len(good), 90)) + bad
    rnd.shuffle(picked)
    buf, recorded = bytearray(rnd.getrandbits(8) for _ in range(16)), []
    for name, prog, z, data in picked:
        recorded.append((8 * len(buf) + H.header_bit(prog), name, H.header_of(prog)[1]))
        buf += z + bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(24, 41)))
    a = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
    nb = 8 * a.size

    def find(which, mis):
        cap = 1 << 18
        out = np.zeros(cap, dtype=np.uint32)
        n = C.c_uint32()
        rc = L.mzhip_find_blocks_host(a.ctypes.data, a.size, 0, nb, which, mis, out.ctypes.data, cap, C.byref(n))
        assert rc == 0 and n.value <= cap, (rc, n.value)
        got = np.sort(out[:n.value])
        assert np.unique(got).size == got.size
        return got

    verdict = {}
    raw = bytes(buf)
    kept_names, dropped = [], {}
    for k, mis in enumerate((0, 1, 2, 3, 5, 8, 15)):
        new, old, kept = find(0, mis), find(1, mis), find(2, mis)
        assert np.array_equal(new, old), (mis, new.size, old.size)
        cands = set(int(p) for p in new)
        keep = set(int(p) for p in kept)
        assert keep <= cands, mis
        for p, name, hdr in recorded:
            if hdr["hlit"] <= 29 and hdr["hdist"] <= 29:
                assert p in cands, (mis, name, p)
        for p in cands:
            if p not in verdict:
                verdict[p] = H.read_header(raw, p)
            v = verdict[p]
            want = v == H.NOT_DYNAMIC or not isinstance(v, str)               # (not dynamic: a stored candidate, kept as it is)
            assert (p in keep) == want, (mis, p, v if isinstance(v, str) else "accepted, ends at bit %d" % v[2], p in keep)
        if k == 0:
            for p, name, hdr in recorded:
                if p in keep:
                    kept_names.append((name, hdr))
                elif p in cands:
                    dropped[verdict[p]] = dropped.get(verdict[p], 0) + 1
            accidental = len(cands) - sum(p in cands for p, _, _ in recorded)
            print("test_header_check_is_exact: %d bytes, %d recorded headers, %d candidates (%d accidental, %d of them kept), %d kept in all; dropped: %s"
                  % (a.size, len(recorded), len(cands), accidental, len(keep) - len(kept_names), len(keep), sorted(dropped.items())))
    assert sum(H.header_bits(h) > 2048 for _, h in kept_names) >= 30
    assert any(T.spelled_lengths(h)[0] == [0] * 256 + [1] for _, h in kept_names)
    assert any("ops/16/crosses_hlit" in n for n, _ in kept_names)
    assert all(dropped.get(r, 0) >= 3 for r in H.REASONS[2:]), dropped
    assert sum(h["hlit"] > 29 or h["hdist"] > 29 for _, _, h in recorded) >= 4     # (too many symbols: never a candidate)
    print("test_header_check_is_exact: %.2f s" % (time.time() - t0))


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "integration", "_build", "libmzhipdrop.so")
ALL = ("rets", "out", "total_in", "total_out", "close", "error", "base_pos", "open")


@pytest.fixture(scope="module")
def libs():
    import importlib

    importlib.import_module("minizip-ng_amd").require_gpu()
    if not os.path.exists(DROP):
        pytest.skip("integration/_build/libmzhipdrop.so missing (built where the reference sources are)")
    if not oracle.have_ref():
        pytest.skip("oracle/_ref/libmzref.so missing (built where the reference sources are)")
    return oracle.MzDriver(DROP), oracle.ref()


def test_header_verdicts_through_the_dropin(libs, entries):
    """400 refused and cut programs by seed through the drop-in's READ stream and through the all-reference build, in 65 535-byte
    and 3-byte read() calls: every read() return value, byte, TOTAL_IN / TOTAL_OUT, close(), error() and the base stream's
    position agree -- TOTAL_IN at the error included (mz_block_code hands back the bit position of each verdict for this)."""
    t0 = time.time()
    hip, ref = libs
    bad = [e for e in entries if e[2] is None]
    bad = random.Random(33).sample(bad, min(400, len(bad)))
    assert sum(e[3] == -3 for e in bad) >= 80 and sum(e[3] == -5 for e in bad) >= 80
    for name, z, _, want in bad:
        for chunk in (65535, 3):
            a = hip.stream_decode(8, z, CAP + 64, chunk=chunk, window_bits=-15)
            b = ref.stream_decode(8, z, CAP + 64, chunk=chunk, window_bits=-15)
            assert {k: a[k] for k in ALL} == {k: b[k] for k in ALL}, (name, chunk, {k: (a[k], b[k]) for k in ALL if a[k] != b[k]})
            assert b["error"] == want or want == -5, (name, b["error"], want)
    print("test_header_verdicts_through_the_dropin: %d programs, %.2f s" % (len(bad), time.time() - t0))
