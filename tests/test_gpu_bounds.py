"""Guard-byte tests: no batch entry point of include/mzhip.h writes outside an entry's own buffers and result words.

Every launch here runs on a batch whose whole output blob holds a seeded byte pattern (tests/gpu_util.make_batch with
fill=), in two layouts: red zones around every entry with odd, unaligned offsets ("zones"), and the packed layout of
bench.py (cap == size, entry i + 1 starts where entry i ends) with red zones in front and behind.  Result arrays have 64
sentinel elements behind the n the call is told.  After every launch gpu_util.check_guards asserts (a) nothing outside a
region was written, (b) the input is unchanged, (c) result elements n .. are untouched and 0 .. n-1 written, (d) a
status-0 entry left [out_len, out_cap) alone -- and EVERY entry's bytes are compared with the host reference (zlib, lzma,
hashlib); the oracle restatement is run on a sample, as elsewhere in the suite."""
import ctypes as C
import hashlib
import lzma as pylzma
import time
import zlib

import numpy as np
import pytest

import oracle
from tests import synth
from tests.synth import fixed_stream, hand_made  # (made by hand: tests/synth.py; tests/asan_bounds.py takes them from here)
from tests.test_oracle import _zip_lzma

pytestmark = pytest.mark.gpu

LAYOUTS = (("zones", dict(guard=67, align=1, odd=True)), ("packed", dict(guard=64, packed=True)))
OUT_FULL = -200
COUNTS = {}


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    t0 = time.time()
    yield gpu_util
    print("\nguarded entries run per entry point (both layouts): %s; %.1f s"
          % (", ".join("%s %d" % kv for kv in sorted(COUNTS.items())), time.time() - t0))


def zlib_inflate(z, cap=None):
    """the host reference: (status class, bytes) of a raw-DEFLATE stream through zlib"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z)
    except zlib.error:
        return -3, b""
    return (0 if d.eof else -5), out


# ---- launch helpers ----------------------------------------------------------------------------------------------------

def _p(t):
    return t.data_ptr() if t is not None else None


def _io(b):
    return (_p(b["d_in"]), _p(b["in_off"]), _p(b["in_len"])), (_p(b["d_out"]), _p(b["out_off"]), _p(b["out_cap"]))


def _sync():
    import torch

    torch.cuda.synchronize()


def _got(gpu, R, n):
    out_len = gpu.result_words(R["out_len"], n).astype(np.int64) if "out_len" in R else np.zeros(n, np.int64)
    status = gpu.result_words(R["status"], n).view(np.int32) if "status" in R else np.zeros(n, np.int32)
    return out_len, status


def _count(what, n):
    COUNTS[what] = COUNTS.get(what, 0) + n


def launch_inflate(gpu, b, resume=None, stop=False):
    n = b["n"]
    names = ("out_len", "in_used", "crc", "status") + (("stop",) if stop else ())
    R = gpu.guarded_results(n, names, words={"stop": 4})
    i, o = _io(b)
    L = gpu.mz.lib()
    if resume is None and not stop:
        rc = L.mzhip_inflate_batch(*i, *o, n, _p(R["out_len"]), _p(R["in_used"]), _p(R["crc"]), _p(R["status"]), None)
        _count("mzhip_inflate_batch", n)
    else:
        rc = L.mzhip_inflate_resume_batch(*i, *o, n, _p(R["out_len"]), _p(R["in_used"]), _p(R["crc"]), _p(R["status"]), _p(resume),
                                          _p(R["stop"]) if stop else None, None)
        _count("mzhip_inflate_resume_batch", n)
    assert rc == 0, gpu.mz.lib().mzhip_last_error()
    _sync()
    return R


def launch_lzma(gpu, b, max_out, xz=False):
    import torch

    n = b["n"]
    R = gpu.guarded_results(n, ("out_len", "in_used", "crc", "status"))
    i, o = _io(b)
    mo = torch.tensor(max_out, dtype=torch.int64, device=b["d_in"].device) if max_out is not None else None
    fn = gpu.mz.lib().mzhip_xz_batch if xz else gpu.mz.lib().mzhip_lzma_batch
    assert fn(*i, *o, _p(mo), n, _p(R["out_len"]), _p(R["in_used"]), _p(R["crc"]), _p(R["status"]), None) == 0
    _count("mzhip_xz_batch" if xz else "mzhip_lzma_batch", n)
    _sync()
    return R


def launch_deflate(gpu, b, final=None, level=None, window=15):
    import torch

    n = b["n"]
    R = gpu.guarded_results(n, ("out_len", "crc", "status"))
    i, o = _io(b)
    fin = torch.tensor(final, dtype=torch.uint8, device=b["d_in"].device) if final is not None else None
    L = gpu.mz.lib()
    if level is None:
        rc = L.mzhip_deflate_batch(*i, *o, _p(fin), n, _p(R["out_len"]), _p(R["crc"]), _p(R["status"]), None)
        _count("mzhip_deflate_batch", n)
    else:
        rc = L.mzhip_deflate_batch_level(*i, *o, _p(fin), n, level, window, _p(R["out_len"]), _p(R["crc"]), _p(R["status"]), None)
        _count("mzhip_deflate_batch_level", n)
    assert rc == 0, L.mzhip_last_error()
    _sync()
    return R


def launch_lzma_encode(gpu, b, mode=None, preset=None):
    import torch

    n = b["n"]
    R = gpu.guarded_results(n, ("out_len", "crc", "status"))
    i, o = _io(b)
    md = torch.tensor(mode, dtype=torch.uint8, device=b["d_in"].device) if mode is not None else None
    mx = int(b["h_in_len"].max()) if n else 0
    L = gpu.mz.lib()
    if preset is None:
        rc = L.mzhip_lzma_encode_batch(*i, mx, *o, _p(md), n, _p(R["out_len"]), _p(R["crc"]), _p(R["status"]), None)
        _count("mzhip_lzma_encode_batch", n)
    else:
        rc = L.mzhip_lzma_encode_batch_preset(*i, mx, *o, _p(md), n, preset, _p(R["out_len"]), _p(R["crc"]), _p(R["status"]), None)
        _count("mzhip_lzma_encode_batch_preset", n)
    assert rc == 0, L.mzhip_last_error()
    _sync()
    return R


def check_decoded(gpu, b, R, want, what, crcs=True, slack_ok=False):
    """guards, then every entry: want[i] = (status, bytes); a status-0 entry's length, bytes and CRC-32, any other entry's
    status (a tuple of statuses: any of them).  -> (host copy of d_out, out_len, status)"""
    n = b["n"]
    out_len, status = _got(gpu, R, n)
    h = gpu.check_guards(b, out_len, status, results=R, words={"stop": 4}, slack_ok=slack_ok)
    crc = gpu.result_words(R["crc"], n)
    for i, (st, data) in enumerate(want):
        if isinstance(st, tuple):
            assert status[i] in st, (what, i, int(status[i]), st)
            continue
        assert status[i] == st, (what, i, int(status[i]), st)
        if st == 0:
            assert out_len[i] == len(data), (what, i, int(out_len[i]), len(data))
            assert gpu.entry_bytes(b, h, i, len(data)) == data, (what, i)
            if crcs:
                assert crc[i] == zlib.crc32(data), (what, i)
    return h, out_len, status


# ---- mzhip_inflate_batch -----------------------------------------------------------------------------------------------

def inflate_cases():
    """(name, stream, expected bytes): everything decodes with zlib to the bytes named"""
    c = synth.corpus()
    cases = [(name, z, data) for name, data, z in synth.edge_payloads()]
    cases += [(name, z, data) for name, data, z in synth.long_code_payloads()]
    cases.append(("stored_1000", synth.stored_blocks(c[:3000], block=1000), c[:3000]))
    for name, z in hand_made():
        st, data = zlib_inflate(z)
        assert st == 0, name
        cases.append((name, z, data))
    for k, d in enumerate(synth.slices(40, 8192, 31) + synth.slices(12, 65536, 32)):
        cases.append(("slice%d" % k, synth.deflate_raw(d, level=(1, 6, 9)[k % 3]), d))
    for name, z, data in cases:
        assert zlib_inflate(z) == (0, data), name
    return cases


def test_inflate_batch_bounds(gpu):
    cases = inflate_cases()
    assert any(len(d) == 0 for _, _, d in cases) and any(n == "ends_in_258_match" for n, _, _ in cases)
    for lname, lay in LAYOUTS:
        for cname, capf, st in (("exact", lambda k: k, 0), ("minus1", lambda k: max(k - 1, 0), OUT_FULL),
                                ("half", lambda k: k // 2, OUT_FULL), ("zero", lambda k: 0, OUT_FULL)):
            pays = [z for _, z, _ in cases]
            caps = [capf(len(d)) for _, _, d in cases]
            # an entry whose bytes fit its cap decodes (the empty streams at every cap, a 1-byte entry at cap 1 // 2 ... not)
            want = [(0 if caps[i] >= len(d) else st, d) for i, (_, _, d) in enumerate(cases)]
            b = gpu.make_batch(pays, caps, fill=100 + len(cname), **lay)
            R = launch_inflate(gpu, b)
            check_decoded(gpu, b, R, want, (lname, cname))
            if cname == "exact":
                in_used = gpu.result_words(R["in_used"], b["n"])
                assert (in_used == np.array([len(p) for p in pays])).all()
                for i in range(0, len(cases), 7):
                    so, uo, oo = oracle.inflate_raw(pays[i], caps[i])
                    assert (so, uo, oo) == (0, len(pays[i]), cases[i][2]), cases[i][0]


def _geometry(gpu):
    g = C.c_uint32()
    w = C.c_uint32()
    gpu.mz.lib().mzhip_inflate_launch_geometry(0x7FFFFFFF, C.byref(g), C.byref(w), None)
    assert g.value > 0 and w.value == 4
    return g.value


def _edge_ns(gpu):
    g = _geometry(gpu)
    return [1, 3, 4, 5, 63, 64, 65, 4 * g - 1, 4 * g, 4 * g + 1, 8 * g + 5]


def _mixed_pool(n, seed):
    """n entries of 300 .. 3000 bytes, every 97th 64 KiB: waves finish out of order"""
    rnd = np.random.RandomState(seed)
    c = synth.corpus()
    sizes = rnd.randint(300, 3001, size=n)
    sizes[96::97] = 65536
    offs = rnd.randint(0, len(c) - 65536, size=n)
    return [c[int(o):int(o) + int(s)] for o, s in zip(offs, sizes)]


def test_batch_size_edges_inflate(gpu):
    ns = _edge_ns(gpu)
    datas = _mixed_pool(max(ns), 5)
    pays = [synth.deflate_raw(d, level=1 + (i % 3) * 4) for i, d in enumerate(datas)]
    for lname, lay in LAYOUTS:
        for n in ns:
            b = gpu.make_batch(pays[:n], [len(d) for d in datas[:n]], fill=200 + n % 50, **lay)
            R = launch_inflate(gpu, b)
            check_decoded(gpu, b, R, [(0, d) for d in datas[:n]], (lname, n))
    for i in range(0, len(datas), 211):
        assert oracle.inflate_raw(pays[i], len(datas[i])) == (0, len(pays[i]), datas[i])
    # n == 0: returns 0 and touches nothing
    b = gpu.make_batch([], [], fill=9, guard=64)
    R = gpu.guarded_results(0, ("out_len", "in_used", "crc", "status"))
    i, o = _io(b)
    assert gpu.mz.lib().mzhip_inflate_batch(*i, *o, 0, _p(R["out_len"]), _p(R["in_used"]), _p(R["crc"]), _p(R["status"]), None) == 0
    _sync()
    gpu.check_guards(b, [], [], results=R)


def test_batch_size_edges_deflate_level1(gpu):
    ns = _edge_ns(gpu)
    datas = _mixed_pool(max(ns), 6)
    for lname, lay in LAYOUTS:
        for n in ns:
            b = gpu.make_batch(datas[:n], [len(d) + len(d) // 8 + 64 for d in datas[:n]], fill=300 + n % 50, **lay)
            R = launch_deflate(gpu, b)
            out_len, status = _got(gpu, R, n)
            h = gpu.check_guards(b, out_len, status, results=R)
            crc = gpu.result_words(R["crc"], n)
            assert (status == 0).all(), (lname, n)
            for i, d in enumerate(datas[:n]):
                z = gpu.entry_bytes(b, h, i, int(out_len[i]))
                assert zlib.decompress(z, -15) == d and crc[i] == zlib.crc32(d), (lname, n, i)
                if i % 211 == 0 and n == ns[-1]:
                    assert oracle.inflate_raw(z, len(d)) == (0, len(z), d)
    b = gpu.make_batch([], [], fill=9, guard=64)
    R = gpu.guarded_results(0, ("out_len", "crc", "status"))
    i, o = _io(b)
    assert gpu.mz.lib().mzhip_deflate_batch(*i, *o, None, 0, _p(R["out_len"]), _p(R["crc"]), _p(R["status"]), None) == 0
    _sync()
    gpu.check_guards(b, [], [], results=R)


def _launch_sum(gpu, b, which, init=None):
    n = b["n"]
    R = gpu.guarded_results(n, (which,))
    i, _ = _io(b)
    L = gpu.mz.lib()
    if which == "crc":
        rc = L.mzhip_crc32_batch(*i, n, _p(init), _p(R["crc"]), None)
        _count("mzhip_crc32_batch", n)
    else:
        rc = L.mzhip_adler32_batch(*i, n, _p(R["adler"]), None)
        _count("mzhip_adler32_batch", n)
    assert rc == 0
    _sync()
    gpu.check_guards(b, [], [], results=R, outputs=False)
    return gpu.result_words(R[which], n)


def test_batch_size_edges_crc32(gpu):
    ns = _edge_ns(gpu)
    datas = _mixed_pool(max(ns), 7)
    want = np.array([zlib.crc32(d) for d in datas], dtype=np.uint32)
    for lname, lay in LAYOUTS:
        for n in ns:
            b = gpu.make_batch(datas[:n], [0] * n, fill=400 + n % 50, **lay)
            got = _launch_sum(gpu, b, "crc")
            assert (got == want[:n]).all(), (lname, n, int(np.flatnonzero(got != want[:n])[0]))
    b = gpu.make_batch([], [], fill=9, guard=64)
    R = gpu.guarded_results(0, ("crc",))
    i, _ = _io(b)
    assert gpu.mz.lib().mzhip_crc32_batch(*i, 0, None, _p(R["crc"]), None) == 0
    _sync()
    gpu.check_guards(b, [], [], results=R, outputs=False)


# ---- checksums and digests ---------------------------------------------------------------------------------------------

def test_checksum_and_digest_bounds(gpu):
    import torch

    rnd = np.random.RandomState(8)
    sizes = [0, 1, 2, 15, 16, 17, 55, 56, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 300001, 0, 3]
    datas = [rnd.bytes(s) for s in sizes]
    for lname, lay in LAYOUTS:
        b = gpu.make_batch(datas, [0] * len(datas), fill=17, **lay)
        init = rnd.randint(0, 2**31, size=len(datas)).astype(np.int32)
        got = _launch_sum(gpu, b, "crc", init=torch.from_numpy(init).to(b["d_in"].device))
        for i, d in enumerate(datas):
            assert got[i] == zlib.crc32(d, int(init[i])) == oracle.crc32(d, int(init[i])), (lname, sizes[i])
        got = _launch_sum(gpu, b, "adler")
        for i, d in enumerate(datas):
            assert got[i] == zlib.adler32(d), (lname, sizes[i])
    # SHA: one lane per buffer, blocks of 256 lanes
    fns = {20: hashlib.sha1, 22: hashlib.sha224, 23: hashlib.sha256, 24: hashlib.sha384, 25: hashlib.sha512}
    pool = [rnd.bytes(int(s)) for s in rnd.randint(0, 300, size=257)]
    for k, s in enumerate((0, 1, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127, 128, 129, 5000)):
        pool[k * 17 % 257] = rnd.bytes(s)
    for lname, lay in LAYOUTS:
        for n in (1, 255, 256, 257):
            b = gpu.make_batch(pool[:n], [0] * n, fill=18 + n, **lay)
            for alg, fn in fns.items():
                w = 16 if alg in (24, 25) else 8
                R = gpu.guarded_results(n, ("digest",), words={"digest": w})
                i, _ = _io(b)
                assert gpu.mz.lib().mzhip_sha_batch(*i, n, alg, _p(R["digest"]), None) == 0
                _count("mzhip_sha_batch", n)
                _sync()
                gpu.check_guards(b, [], [], results=R, words={"digest": w}, outputs=False)
                dg = gpu.result_words(R["digest"], n, w).view(np.uint8).reshape(n, 4 * w)
                for k in range(n):
                    want = fn(pool[k]).digest()
                    assert dg[k].tobytes() == want + bytes(4 * w - len(want)), (lname, n, alg, k)


# ---- mzhip_inflate_resume_batch ----------------------------------------------------------------------------------------

def test_inflate_resume_batch_bounds(gpu):
    """Streams decoded window by window (300, 4096 and 65 536 bytes of room behind at most 32 KiB of history): every launch on a
    freshly patterned blob; the history bytes in front of each region come back unchanged, the stop states are written
    for n entries only, and the windows concatenate to zlib's bytes.  A call that ends with OUT_FULL has
    made progress -- a byte or a bit -- whenever the next token fits the room: the step loop writes what fits of its queue of
    up to 64 tokens (csrc/inflate_flush.inc; it used to write all 16 512 bytes of it or none, and 60 of 81 streams stood
    still with 300 bytes of room, three run streams with 4 096)."""
    import torch

    # A stored block is one token (include/mzhip.h): the room must hold it whole.  zlib stores what does not compress (the noise
    # of these three cases, in blocks of up to 65 535 bytes); the streams of stored blocks made here say their block size.
    c = synth.corpus()
    room = {"random_incompressible": 65535, "max_distance": 65535, "stored_only": 65535, "stored_1000": 1000}
    cases = [(n, z, d) for n, z, d in inflate_cases() if len(d) <= 70000]
    cases.append(("stored_250", synth.stored_blocks(c[:3000], block=250), c[:3000]))
    stalled = []
    for lname, lay in LAYOUTS:
        for window in (300, 4096, 65536):
            todo = [i for i in range(len(cases)) if room.get(cases[i][0], 258) <= window]
            assert len(todo) >= len(cases) - 4 and (window < 65536 or len(todo) == len(cases))
            got = {i: bytearray() for i in todo}
            state = {i: (0, 0, 0, 0) for i in todo}
            rounds = 0
            while todo:
                rounds += 1
                assert rounds < 400
                hist = [state[i][2] for i in todo]
                b = gpu.make_batch([cases[i][1] for i in todo], [h + window for h in hist], fill=500 + rounds, **lay)
                h0 = b["h_fill"].copy()
                for k, i in enumerate(todo):
                    o = int(b["h_out_off"][k])
                    if hist[k]:
                        h0[o:o + hist[k]] = np.frombuffer(bytes(got[i][-hist[k]:]), dtype=np.uint8)
                b["d_out"].copy_(torch.from_numpy(h0))
                res = torch.tensor([state[i] for i in todo], dtype=torch.int64).to(torch.int32).to(b["d_in"].device)
                R = launch_inflate(gpu, b, resume=res, stop=True)
                n = b["n"]
                out_len, status = _got(gpu, R, n)
                # the history is the caller's: (d) is checked against a pattern that holds it
                b["h_fill"] = h0
                h = gpu.check_guards(b, out_len, status, results=R, words={"stop": 4})
                stop = gpu.result_words(R["stop"], n, 4)
                nxt = []
                for k, i in enumerate(todo):
                    o = int(b["h_out_off"][k])
                    assert (h[o:o + hist[k]] == h0[o:o + hist[k]]).all(), (lname, window, i, "history changed")
                    assert status[k] in (0, OUT_FULL), (lname, window, cases[i][0], int(status[k]))
                    valid = int(out_len[k]) if status[k] == 0 else int(stop[k][2])
                    assert hist[k] <= valid <= hist[k] + window, (lname, window, i, valid)
                    got[i] += h[o + hist[k]:o + valid].tobytes()
                    if status[k] == 0:
                        assert bytes(got[i]) == cases[i][2], (lname, window, cases[i][0])
                        continue
                    assert stop[k][3] & 1, (lname, window, cases[i][0])
                    if valid == hist[k] and (int(stop[k][0]), int(stop[k][1])) == state[i][:2]:
                        stalled.append((lname, window, cases[i][0], len(got[i])))        # OUT_FULL, and neither a byte nor a bit further
                        continue
                    state[i] = (int(stop[k][0]), int(stop[k][1]), min(len(got[i]), 32768), 1)
                    nxt.append(i)
                todo = nxt
    print("resume: %d stalled (layout, window, stream, bytes decoded before): %s" % (len(stalled), stalled))
    assert not stalled, "%d streams stop with OUT_FULL and make no progress although the next token fits the room: %s" % (len(stalled), stalled[:12])


# ---- mzhip_inflate_large -----------------------------------------------------------------------------------------------

def test_inflate_large_bounds(gpu):
    import torch

    text, _ = synth.bench_corpus()
    rnd = np.random.RandomState(2)
    d = b""
    while len(d) < 6 << 20:
        d += text[:1500000] + rnd.bytes(300000) + bytes(700000) + text[::-1][:900000]
    d += text[:55555]
    assert 5 << 20 <= len(d) <= 10 << 20
    z = synth.deflate_raw(d, 6)
    G = 4096
    dev = torch.device("cuda", 0)
    L = gpu.mz.lib()
    h_in = gpu.guard_pattern(G + len(z) + G, 71)
    h_in[G:G + len(z)] = np.frombuffer(z, dtype=np.uint8)
    for cap in (len(d), len(d) - 1):
        d_in = torch.from_numpy(h_in).to(dev)
        h_fill = gpu.guard_pattern(G + cap + G, 72)
        d_out = torch.from_numpy(h_fill.copy()).to(dev)
        ol, iu, ck, st = C.c_uint32(SENT), C.c_uint32(SENT), C.c_uint32(SENT), C.c_int32(0x5EED)
        assert L.mzhip_inflate_large(d_in.data_ptr() + G, len(z), d_out.data_ptr() + G, cap, C.byref(ol), C.byref(iu), C.byref(ck),
                                     C.byref(st), None) == 0
        _sync()
        _count("mzhip_inflate_large", 1)
        h = d_out.cpu().numpy()
        for name, lo, hi in (("in front of", 0, G), ("behind", G + cap, G + cap + G)):
            bad = np.flatnonzero(h[lo:hi] != h_fill[lo:hi])
            assert bad.size == 0, "cap %d: byte %d %s the buffer was written (%d bytes)" % (cap, int(bad[0]) - (G if lo == 0 else 0), name, bad.size)
        assert (d_in.cpu().numpy() == h_in).all(), "input changed"
        if cap == len(d):
            assert (st.value, ol.value, iu.value, ck.value) == (0, len(d), len(z), zlib.crc32(d))
            assert h[G:G + cap].tobytes() == d
        else:
            assert st.value == OUT_FULL and ol.value <= cap and h[G:G + ol.value].tobytes() == d[:ol.value], (st.value, ol.value)


SENT = 0x5EED5EED


# ---- mzhip_lzma_batch / mzhip_xz_batch ---------------------------------------------------------------------------------

def lzma_cases():
    """(name, ZIP method-14 payload, bytes): the lc / lp / pb classes of both kernels -- text at lc3 stays in the slot kernel,
    noise and lp4 are given back to the full-model kernel (tests/test_kernel_emul.test_lzma_slot_build)"""
    c = synth.corpus()
    rnd = np.random.RandomState(4)
    noise = rnd.bytes(20000)
    base = [("empty", b""), ("one", b"a"), ("text", c[:60000]), ("noise", noise), ("run", b"A" * 30000),
            ("mixed", c[1000:20000] + noise[:3000] + c[:15000])] + [("slice%d" % k, d) for k, d in enumerate(synth.slices(12, 8192, 41))]
    cases = []
    for name, d in base:
        for lc, lp, pb in ((3, 0, 2), (0, 0, 2), (4, 0, 0), (1, 2, 2), (0, 4, 1)):
            if name.startswith("slice") and (lc, lp, pb) != (3, 0, 2):
                continue
            raw = pylzma.compress(d, format=pylzma.FORMAT_ALONE, filters=[dict(id=pylzma.FILTER_LZMA1, preset=6, lc=lc, lp=lp, pb=pb)])
            assert pylzma.decompress(raw, format=pylzma.FORMAT_ALONE) == d
            cases.append(("%s lc%d lp%d pb%d" % (name, lc, lp, pb), bytes([5, 2, 5, 0]) + raw[:5] + raw[13:], d))
    for k, d in enumerate(synth.slices(6, 8192, 42)):
        cases.append(("zip%d" % k, _zip_lzma(d), d))
    return cases


def _coder_bounds(gpu, cases, xz):
    what = "xz" if xz else "lzma"
    for lname, lay in LAYOUTS:
        pays = [z for _, z, _ in cases]
        lens = [len(d) for _, _, d in cases]
        # exact cap: with the size known (PROP_TOTAL_OUT_MAX) and without
        for mo in (lens, None):
            b = gpu.make_batch(pays, lens, fill=600, **lay)
            R = launch_lzma(gpu, b, mo, xz)
            check_decoded(gpu, b, R, [(0, d) for _, _, d in cases], (what, lname, "exact", mo is None))
            in_used = gpu.result_words(R["in_used"], b["n"])
            assert (in_used == np.array([len(p) for p in pays])).all(), (what, lname)
        # cap - 1
        caps = [max(k - 1, 0) for k in lens]
        b = gpu.make_batch(pays, caps, fill=601, **lay)
        R = launch_lzma(gpu, b, [-1] * len(cases), xz)
        check_decoded(gpu, b, R, [(OUT_FULL if len(d) else 0, d) for _, _, d in cases], (what, lname, "cap-1"))
        # the clamp below the stream's length (include/mzhip.h): the stream is still decoded to its end inside out_cap, length
        # and CRC cover the prefix -- so (d) is not this call's contract (slack_ok), (a) is, and in the packed layout every
        # neighbour's bytes are compared: the bytes behind the clamp stay inside the entry's own out_cap
        clamp = [k * 2 // 3 for k in lens]
        b = gpu.make_batch(pays, lens, fill=602, **lay)
        R = launch_lzma(gpu, b, clamp, xz)
        check_decoded(gpu, b, R, [(0, d[:clamp[i]]) for i, (_, _, d) in enumerate(cases)], (what, lname, "clamp"), slack_ok=True)
        # ... and into out_cap == clamp: a stream that produces more than its out_cap is OUT_FULL
        b = gpu.make_batch(pays, clamp, fill=603, **lay)
        R = launch_lzma(gpu, b, clamp, xz)
        check_decoded(gpu, b, R, [(0 if len(d) <= clamp[i] else OUT_FULL, d) for i, (_, _, d) in enumerate(cases)], (what, lname, "clamp == cap"))
    for i in range(0, len(cases), 9):
        name, z, d = cases[i]
        assert (oracle.xz_decode(z, len(d)) if xz else oracle.lzma_zip_decode(z, len(d), len(d))) == (0, len(z), d), name


def test_lzma_batch_bounds(gpu):
    _coder_bounds(gpu, lzma_cases(), False)


def test_xz_batch_bounds(gpu):
    cases = [(name, x, d) for name, d, x in synth.xz_cases()]
    for name, x, d in cases:
        assert pylzma.decompress(x) == d, name
    _coder_bounds(gpu, cases, True)


# ---- mzhip_deflate_batch / _level --------------------------------------------------------------------------------------

ENC_SIZES = (0, 1, 2, 63, 64, 65, 16383, 16384, 16385, 65535, 65536, 65537)


def _enc_inputs():
    c = synth.corpus()
    rnd = np.random.RandomState(13)
    return [c[7:7 + s] for s in ENC_SIZES] + [b"A" * 70000, b"ab" * 9000], [rnd.bytes(s) for s in ENC_SIZES]


def test_deflate_batch_bounds(gpu):
    text, noise = _enc_inputs()
    datas = text + noise
    final = [1 - (i % 3 == 1) for i in range(len(datas))]                      # every third piece non-final
    for lname, lay in LAYOUTS:
        for level, window in ((None, 15), (1, 15), (1, 9), (6, 15), (6, 9), (9, 15), (9, 9)):
            b = gpu.make_batch(datas, [len(d) + len(d) // 8 + 64 for d in datas], fill=700, **lay)
            R = launch_deflate(gpu, b, final=final, level=level, window=window)
            out_len, status = _got(gpu, R, b["n"])
            h = gpu.check_guards(b, out_len, status, results=R)
            crc = gpu.result_words(R["crc"], b["n"])
            assert (status == 0).all(), (lname, level, window, status.tolist())
            for i, d in enumerate(datas):
                z = gpu.entry_bytes(b, h, i, int(out_len[i]))
                dec = zlib.decompressobj(-window)
                assert dec.decompress(z) == d and dec.eof == bool(final[i]) and crc[i] == zlib.crc32(d), (lname, level, window, i)
                if i % 5 == 0 and final[i]:
                    assert oracle.inflate_raw(z, len(d)) == (0, len(z), d)
            # incompressible input into cap == len and cap == len // 4: OUT_FULL, nothing outside
            for capf in (lambda k: k, lambda k: k // 4):
                b = gpu.make_batch(noise, [capf(len(d)) for d in noise], fill=701, **lay)
                R = launch_deflate(gpu, b, level=level, window=window)
                out_len, status = _got(gpu, R, b["n"])
                gpu.check_guards(b, out_len, status, results=R)
                assert (status == OUT_FULL).all(), (lname, level, window, status.tolist())


# ---- mzhip_lzma_encode_batch / _preset, the LZMA2 chunk coder through mzhip_xz_encode_host ----------------------------

def _unwrap_lzma(z, mode, n):
    if mode == 0:
        return pylzma.decompress(z[4:9] + b"\xff" * 8 + z[9:], format=pylzma.FORMAT_ALONE)
    if n == 0:
        return b""
    body = bytes([0xE0 | ((n - 1) >> 16), ((n - 1) >> 8) & 255, (n - 1) & 255, (len(z) - 1) >> 8, (len(z) - 1) & 255, 0x5D]) + z + b"\x00"
    return pylzma.decompress(body, format=pylzma.FORMAT_RAW, filters=[{"id": pylzma.FILTER_LZMA2, "dict_size": 8 << 20}])


def test_lzma_encode_batch_bounds(gpu):
    text, noise = _enc_inputs()
    datas = text + noise
    # mode 1 (the payload of one LZMA2 chunk) where a chunk can hold it: compressible, at most 64 KiB
    mode = [1 if (i % 2 and 0 < len(d) <= 65536 and i < len(text)) else 0 for i, d in enumerate(datas)]
    for lname, lay in LAYOUTS:
        for preset in (None, 1, 6):
            b = gpu.make_batch(datas, [len(d) + len(d) // 8 + 1024 for d in datas], fill=800, **lay)
            R = launch_lzma_encode(gpu, b, mode=mode, preset=preset)
            out_len, status = _got(gpu, R, b["n"])
            h = gpu.check_guards(b, out_len, status, results=R)
            crc = gpu.result_words(R["crc"], b["n"])
            assert (status == 0).all(), (lname, preset, status.tolist())
            for i, d in enumerate(datas):
                z = gpu.entry_bytes(b, h, i, int(out_len[i]))
                assert _unwrap_lzma(z, mode[i], len(d)) == d and crc[i] == zlib.crc32(d), (lname, preset, i, mode[i])
                if i % 5 == 0 and mode[i] == 0:
                    assert oracle.lzma_zip_decode(z, len(d) + 64, -1) == (0, len(z), d)
            for capf in (lambda k: k, lambda k: k // 4):
                b = gpu.make_batch(noise, [capf(len(d)) for d in noise], fill=801, **lay)
                R = launch_lzma_encode(gpu, b, preset=preset)
                out_len, status = _got(gpu, R, b["n"])
                gpu.check_guards(b, out_len, status, results=R)
                assert (status == OUT_FULL).all(), (lname, preset, status.tolist())


def test_xz_encode_host_bounds(gpu):
    """The LZMA2 chunk coder has no batch entry point: through mzhip_xz_encode_host into a patterned host buffer"""
    text, noise = _enc_inputs()
    L = gpu.mz.lib()
    G = 256
    text = text + [synth.corpus()[:200000]]
    for k, d in enumerate(text + noise):
        for cap in (len(d) + len(d) // 8 + 1024, len(d) // 4, 11):
            fill = gpu.guard_pattern(G + cap + G, 900 + k)
            buf = fill.copy()
            src = np.frombuffer(d, dtype=np.uint8).copy() if d else np.zeros(1, np.uint8)
            keep = src.copy()
            ol, crc = C.c_uint32(0), C.c_uint32(0)
            rc = L.mzhip_xz_encode_host(src.ctypes.data, len(d), buf.ctypes.data + G, cap, C.byref(ol), C.byref(crc))
            _count("mzhip_xz_encode_host", 1)
            assert (buf[:G] == fill[:G]).all() and (buf[G + cap:] == fill[G + cap:]).all(), (k, cap, "red zone written")
            assert (src == keep).all()
            if cap == 11 or (cap < len(d) and k >= len(text)):          # less than a stream header; noise into a quarter of its size
                assert rc == OUT_FULL, (k, cap, rc)
            elif cap > len(d):
                assert rc == 0, (k, cap, rc)
            if rc == 0:
                assert ol.value <= cap and crc.value == zlib.crc32(d), (k, rc)
                assert pylzma.decompress(buf[G:G + ol.value].tobytes()) == d, k
                assert (buf[G + ol.value:G + cap] == fill[G + ol.value:G + cap]).all(), (k, "bytes behind out_len written")
            else:
                assert rc == OUT_FULL, (k, cap, rc)                       # (text that does not fit a quarter of its size)


# ---- isolation ---------------------------------------------------------------------------------------------------------

def test_inflate_isolation_of_failing_entries(gpu):
    """2000 good entries decoded; then every third replaced in place by a broken one and decoded again into a freshly
    patterned blob: the untouched entries give the same bytes and result words, the guards hold, and an entry whose
    distance reaches in front of its own output is refused (-3) before anything of its neighbour is copied."""
    n = 2000
    datas = synth.slices(n, 8192, 77)
    good = [synth.deflate_raw(d) for d in datas]
    far0 = fixed_stream([(258, 1), 65, 66])                                  # the first token is a match
    far100 = fixed_stream(list(datas[0][:100]) + [(258, 32768), 67])       # distance 32 768 at output position 100
    assert zlib_inflate(far0)[0] == -3 and zlib_inflate(far100)[0] == -3
    pays, caps, want = list(good), [8192] * n, [(0, d) for d in datas]
    kinds = {}
    for j, i in enumerate(range(1, n, 3)):
        k = j % 5
        kinds[i] = k
        if k == 0:
            pays[i] = good[i][:len(good[i]) // 2]
            want[i] = (-5, None)
        elif k == 1:
            zz = bytearray(good[i])
            zz[len(zz) // 3] ^= 0x10
            pays[i] = bytes(zz)
            st, out = zlib_inflate(pays[i])
            want[i] = (0, out) if st == 0 and len(out) <= 8192 else ((-3, -5, OUT_FULL), None)
        elif k == 2:
            pays[i], want[i] = far0, (-3, None)
        elif k == 3:
            pays[i], want[i] = far100, (-3, None)
        else:
            caps[i], want[i] = 4000, (OUT_FULL, None)
    for lname, lay in LAYOUTS:
        b1 = gpu.make_batch(good, [8192] * n, fill=1000, **lay)
        R1 = launch_inflate(gpu, b1)
        h1, _, _ = check_decoded(gpu, b1, R1, [(0, d) for d in datas], (lname, "good"))
        b2 = gpu.make_batch(pays, caps, fill=1001, **lay)
        R2 = launch_inflate(gpu, b2)
        h2, out_len, status = check_decoded(gpu, b2, R2, want, (lname, "mixed"))
        for name in ("out_len", "in_used", "crc", "status"):
            a, c = gpu.result_words(R1[name], n), gpu.result_words(R2[name], n)
            same = [i for i in range(n) if i not in kinds]
            assert (a[same] == c[same]).all(), (lname, name)
        for i, k in kinds.items():
            if k in (2, 3):
                o = int(b2["h_out_off"][i])
                keep = 0 if k == 2 else 100                                   # the literals in front of the refused match
                # where the 258 bytes of the refused match would lie: nothing was copied, from the neighbour or anywhere else
                assert (h2[o + keep:o + keep + 258] == b2["h_fill"][o + keep:o + keep + 258]).all(), (lname, i, "bytes copied before the refusal")


def test_lzma_isolation_of_failing_entries(gpu):
    """the same for LZMA: a first packet that is a match (rep0 beyond the empty dictionary) between good entries"""
    n = 300
    datas = synth.slices(n, 8192, 78)
    good = [_zip_lzma(d) for d in datas]
    # a stream whose first packet is a match: liblzma refuses it, so does the oracle
    bad = None
    for seed in range(200):
        rnd = np.random.RandomState(seed)
        cand = good[0][:9] + b"\x00" + rnd.bytes(40)
        if oracle.lzma_zip_decode(cand, 8192, -1)[0] == -3 and oracle.lzma_zip_decode(cand, 8192, -1)[2] == b"":
            bad = cand
            break
    assert bad is not None
    pays, want = list(good), [(0, d) for d in datas]
    for i in range(1, n, 3):
        pays[i], want[i] = bad, ((-3, -5), None)
    for lname, lay in LAYOUTS:
        b1 = gpu.make_batch(good, [8192] * n, fill=1100, **lay)
        R1 = launch_lzma(gpu, b1, [8192] * n)
        check_decoded(gpu, b1, R1, [(0, d) for d in datas], (lname, "good"))
        b2 = gpu.make_batch(pays, [8192] * n, fill=1101, **lay)
        R2 = launch_lzma(gpu, b2, [8192] * n)
        h2, _, _ = check_decoded(gpu, b2, R2, want, (lname, "mixed"))
        same = [i for i in range(n) if i % 3 != 1]
        for name in ("out_len", "in_used", "crc", "status"):
            assert (gpu.result_words(R1[name], n)[same] == gpu.result_words(R2[name], n)[same]).all(), (lname, name)
        for i in range(1, n, 3):
            o = int(b2["h_out_off"][i])
            assert (h2[o:o + 64] == b2["h_fill"][o:o + 64]).all(), (lname, i)
