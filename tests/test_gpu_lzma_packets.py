"""GPU tests of the packet programs (tests/lzma_packets.py): LZMA1 / LZMA2 streams written packet by packet -- every edge of
the state graph, every length and slot, reps before a distance was set, distances at the dictionary's edge, overlap copies
at every alignment, every literal context, streams that make K3's slot build swap and give entries back, compressed
lengths on every residue of the 256-byte input window, packets trained to cost 14 bytes, every LZMA2 control byte --
through mzhip_lzma_batch and mzhip_xz_batch and through the windowed host entry points.  liblzma is the judge
(tests/test_lzma_packets.py holds the writer and the oracle restatement against it on the CPU).

Caps of this file: at most 4096 entries and 64 MiB of expected output per launch, no entry above 256 KiB -- except the named
large entries (distance-1 runs of 1, 2 and 4 MiB that reach slot 43; LZMA2 chunks of k * 64 KiB + 1 bytes, which the size
bits of a control byte ask for, up to the largest chunk of 2 MiB), which go in launches of their own.  K3 is one serial
chain per wave: 10.34 GiB/s over about 4096 resident waves (README, config 4) is some 2.5 MB/s per wave, so a 256 KiB
entry takes about 0.1 s and a 4 MiB entry under 2 s."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import oracle
from tests import lzma_packets as K

pytestmark = pytest.mark.gpu

MAX_ENTRIES, MAX_LAUNCH_BYTES, MAX_ENTRY_BYTES = 4096, 64 << 20, 256 << 10
CHECKS = (0, 1, 4, 10)


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    L = gpu_util.mz.lib()
    for fn in (L.mzhip_lzma_batch, L.mzhip_xz_batch):
        fn.restype = C.c_int32
        fn.argtypes = [C.c_void_p] * 7 + [C.c_uint32] + [C.c_void_p] * 5
    return gpu_util


def _launch(gpu, which, entries, caps, large=False, **layout):
    """entries: [(name, stream, bytes or None)] -> the batch, its output buffer and per-entry results of ONE launch"""
    import torch

    nbytes = sum(len(e[2]) for e in entries if e[2])
    assert len(entries) <= MAX_ENTRIES and nbytes <= MAX_LAUNCH_BYTES
    assert large or all(len(e[2]) <= MAX_ENTRY_BYTES for e in entries if e[2])
    b = gpu.make_batch([e[1] for e in entries], caps, **layout)
    n = len(entries)
    dev = b["d_in"].device
    out_len, in_used, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    mo = torch.full((n,), -1, dtype=torch.int64, device=dev)
    fn = gpu.mz.lib().mzhip_lzma_batch if which == 14 else gpu.mz.lib().mzhip_xz_batch
    rc = fn(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), b["d_out"].data_ptr(), b["out_off"].data_ptr(),
            b["out_cap"].data_ptr(), mo.data_ptr(), n, out_len.data_ptr(), in_used.data_ptr(), crc.data_ptr(), status.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return b, b["d_out"].cpu().numpy(), (out_len.cpu().numpy(), in_used.cpu().numpy(), gpu.mz.u32(crc), status.cpu().numpy())


def _check_good(gpu, what, batch, h_out, res, i, name, z, data):
    out_len, in_used, crc, status = res
    assert status[i] == 0, (what, name, int(status[i]))
    used = len(z) if z[:4] == b"\x05\x02\x05\x00" else len(z) & ~3      # (an .xz stream is whole words: what is more is the tail _xz adds)
    assert out_len[i] == len(data) and in_used[i] == used, (what, name, int(out_len[i]), len(data), int(in_used[i]), used)
    got = gpu.entry_bytes(batch, h_out, i, len(data))
    if got != data:
        bad = next(k for k in range(len(data)) if got[k] != data[k])
        raise AssertionError("%s: %s: byte %d of %d is %d, expand() says %d" % (what, name, bad, len(data), got[bad], data[bad]))
    assert int(crc[i]) == zlib.crc32(data), (what, name)


def _three_layouts(gpu, which, test, entries):
    """ONE launch with the entries laid out byte by byte; once more packed, so that input and output misalignments take every
    value and an overrun lands in a neighbour; once more in a seeded shuffled order.  out_cap exact for every second entry."""
    total = sum(len(d) for _, _, d in entries)
    print("%s: %d entries, %d bytes of expected output per launch, largest entry %d" % (test, len(entries), total, max(len(d) for _, _, d in entries)))
    caps = [len(d) + (0 if i % 2 == 0 else 1 + (i * 7) % 64) for i, (_, _, d) in enumerate(entries)]
    order = list(range(len(entries)))
    random.Random(30).shuffle(order)
    for what, idx, layout in (("align=1", None, dict(align=1)), ("packed", None, dict(packed=True)), ("shuffled", order, dict(align=1))):
        es = entries if idx is None else [entries[k] for k in idx]
        cs = caps if idx is None else [caps[k] for k in idx]
        batch, h_out, res = _launch(gpu, which, es, cs, **layout)
        if what == "packed":
            assert len({int(o) & 15 for o in batch["h_out_off"]}) == 16 and len({int(o) & 3 for o in batch["h_in_off"]}) == 4
        for i, (name, z, data) in enumerate(es):
            _check_good(gpu, what, batch, h_out, res, i, name, z, data)


def _accepted14():
    return [(p.name, p.zip14(), d) for p, d in K.accepted()] + [(p.name, p.zip14(), bytes(p.expand()[0])) for p, cap, st, n in K.out_cap_cases() if st == 0]


def _xz(p, i):
    """the program framed with check type i mod 4, and i mod 4 bytes behind the stream that are not its own: in a packed batch
    the streams then start at every misalignment"""
    return p.xz(CHECKS[i % 4]) + b"\x5a" * (i % 4 if i % 8 < 4 else (i + 1) % 4)


def _chunk_entries(large):
    out = []
    for i, p in enumerate(K.chunk_programs()):
        want, verdict = p.expand()
        if (verdict is None or verdict[0] == "end") and (len(want) > MAX_ENTRY_BYTES) == large:
            out.append((p.name, _xz(p, i), bytes(want)))
    return out


def test_batch_packet_programs(gpu):
    """every accepted method-14 program of every family in one mzhip_lzma_batch launch, in three layouts: per entry status 0,
    out_len, in_used == len(stream), the bytes and the CRC-32 against expand() / zlib"""
    entries = _accepted14()
    for fam in K.FAMILIES:
        assert any(n.startswith(fam) for n, _, _ in entries), fam
    assert len(entries) >= 190
    _three_layouts(gpu, 14, "test_batch_packet_programs", entries)


def test_batch_chunk_programs(gpu):
    """every accepted chunk program up to 256 KiB, framed into a one-block .xz with each check type, in one mzhip_xz_batch
    launch, in three layouts"""
    entries = _chunk_entries(False)
    assert len(entries) >= 100 and {x[7] for _, x, _ in entries} == set(CHECKS)
    _three_layouts(gpu, 95, "test_batch_chunk_programs", entries)


def test_large_entries(gpu):
    """the named entries above 256 KiB, in launches of their own: distance-1 runs of 1, 2 and 4 MiB with distances up to slot
    43 behind them (method 14); LZMA2 chunks of k * 64 KiB + 1 bytes for the control bytes whose size bits are k, as first and
    as second chunk, the largest chunk (2 MiB) among them (.xz), in launches of at most 60 MiB"""
    big = [(p.name, p.zip14(), bytes(p.expand()[0])) for p in K.big_programs()]
    print("test_large_entries: method 14: %d entries, %d bytes" % (len(big), sum(len(d) for _, _, d in big)))
    assert len(big) == 3 and max(len(d) for _, _, d in big) <= (4 << 20) + 1024
    batch, h_out, res = _launch(gpu, 14, big, [len(d) + i for i, (_, _, d) in enumerate(big)], large=True, align=1)
    for i, (name, z, d) in enumerate(big):
        _check_good(gpu, "large", batch, h_out, res, i, name, z, d)
    big = _chunk_entries(True)
    assert 140 <= len(big) <= 160 and max(len(d) for _, _, d in big) <= (2 << 20) + 1024
    launches, cur = [], []
    for e in big:                          # launches of at most 60 MiB of expected output
        if cur and sum(len(d) for _, _, d in cur) + len(e[2]) > (60 << 20):
            launches.append(cur)
            cur = []
        cur.append(e)
    launches.append(cur)
    assert len(launches) <= 4
    for es in launches:
        print("test_large_entries: .xz: %d entries, %d bytes" % (len(es), sum(len(d) for _, _, d in es)))
        batch, h_out, res = _launch(gpu, 95, es, [len(d) + i % 2 for i, (_, _, d) in enumerate(es)], large=True, align=1)
        for i, (name, z, d) in enumerate(es):
            _check_good(gpu, "large", batch, h_out, res, i, name, z, d)


def _mixed(gpu, which, test, bad, good):
    """one bad entry to three good neighbours in ONE launch: the verdicts are the oracle's, every good neighbour is exact"""
    random.Random(31).shuffle(good)
    entries, caps, want = [], [], []
    for i, (n, z, cap) in enumerate(bad):
        st, _, oo = oracle.lzma_zip_decode(z, cap, -1) if which == 14 else oracle.xz_decode(z, cap)
        assert st in (-3, -200), (n, st)
        entries.append((n, z, None))
        caps.append(cap)
        want.append((st, oo))
        for n2, z2, d2 in good[(3 * i) % (len(good) - 3):][:3]:
            entries.append((n2, z2, d2))
            caps.append(len(d2) + i % 2)
            want.append((0, d2))
    print("%s: %d entries (%d refused), %d bytes of expected output" % (test, len(entries), len(bad), sum(len(e[2]) for e in entries if e[2])))
    batch, h_out, res = _launch(gpu, which, entries, caps, align=1)
    for i, (name, z, data) in enumerate(entries):
        if want[i][0]:
            assert res[3][i] == want[i][0], (name, int(res[3][i]), want[i][0])
            if want[i][0] == -200:            # the cut copy: the bytes up to out_cap are there
                assert res[0][i] == caps[i] and gpu.entry_bytes(batch, h_out, i, caps[i]) == want[i][1], name
        else:
            _check_good(gpu, test, batch, h_out, res, i, name, z, data)


def test_refused_twins(gpu):
    """the refused twins of every family and the out_cap - 1 forms (-200), one bad entry to three good ones, through
    mzhip_lzma_batch; the refused chunk programs through mzhip_xz_batch"""
    bad = [(p.name, p.zip14(), len(p.expand()[0]) + 50) for p in K.refused()]
    bad += [(p.name, p.zip14(), cap) for p, cap, st, n in K.out_cap_cases() if st == -200]
    good = [e for e in _accepted14() if len(e[2]) <= 70000]
    assert len(bad) >= 140
    _mixed(gpu, 14, "test_refused_twins (method 14)", bad, good)
    bad = []
    for i, p in enumerate(K.chunk_programs()):
        want, verdict = p.expand()
        if not (verdict is None or verdict[0] == "end"):
            bad.append((p.name, _xz(p, i), len(want) + 40))
    good = [e for e in _chunk_entries(False) if len(e[2]) <= 70000]
    assert len(bad) >= 300
    _mixed(gpu, 95, "test_refused_twins (.xz)", bad, good)


def test_retry_flood(gpu):
    """one launch in which more entries are given back by the slot build than there are resident waves (cu_count * 10): the
    retry list is longer than the second kernel's grid.  Five contexts in rotation (given back at the 65th swap), and the
    programs that cross the swap allowance late, behind up to 200 KB the full-model kernel must redo"""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    progs = {p.name: p for p in K.family("slots")}
    rot5 = progs["slots/rot5"]
    n = min(cus * 10 + 300, MAX_ENTRIES - 40)
    assert n > cus * 10
    entries = [(rot5.name, rot5.zip14(), bytes(rot5.expand()[0]))] * n
    late = [p for p in K.family("slots") if p.note.get("late")]
    for k in range(30):
        p = late[k % len(late)]
        entries.insert(k * 97, (p.name, p.zip14(), bytes(p.expand()[0])))
    assert all(K.predict_slots(p)[0] for p in late + [rot5])
    print("test_retry_flood: %d entries given back (%d compute units), %d bytes of expected output" % (len(entries), cus, sum(len(e[2]) for e in entries)))
    batch, h_out, res = _launch(gpu, 14, entries, [len(d) + i % 2 for i, (_, _, d) in enumerate(entries)], align=1)
    for i, (name, z, d) in enumerate(entries):
        _check_good(gpu, "flood", batch, h_out, res, i, name, z, d)


class _Lzma2Run:
    """mzhip_lzma2_run_host behind the signature of the emulation's emul_lzma2_run"""
    argtypes = None

    def __init__(self, L):
        class Args(C.Structure):
            _fields_ = [("size", C.c_uint32), ("in_len", C.c_uint32), ("buf_cap", C.c_uint32), ("reserved", C.c_uint32), ("inp", C.c_void_p),
                        ("buf", C.c_void_p), ("state_in", C.c_void_p), ("state_out", C.c_void_p), ("model", C.c_void_p), ("out_len", C.c_void_p),
                        ("in_used", C.c_void_p)]
        self.L, self.Args = L, Args
        L.mzhip_lzma2_run_host.restype = C.c_int32
        L.mzhip_lzma2_run_host.argtypes = [C.POINTER(Args)]

    def __call__(self, src, n, buf, room, st_in, st_out, model, ol, iu):
        a = self.Args(C.sizeof(self.Args), n, room, 0, C.addressof(src), C.addressof(buf), C.addressof(st_in), C.addressof(st_out),
                      C.addressof(model), C.addressof(ol._obj), C.addressof(iu._obj))
        return self.L.mzhip_lzma2_run_host(C.byref(a))


class _HostAsEmul:
    """the windowed host entry points behind the names the window drivers of tests/test_kernel_emul.py call"""

    def __init__(self, L):
        L.mzhip_lzma_model_bytes.restype = C.c_uint32
        L.mzhip_lzma_resume_host.restype = C.c_int32
        L.mzhip_lzma_resume_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        self.L = L
        self.emul_lzma2_run = _Lzma2Run(L)

    def emul_lzma_model_u16(self):
        return self.L.mzhip_lzma_model_bytes() // 2

    def emul_lzma_resume(self, src, n, buf, cap, st, sto, model, ol, iu):
        return self.L.mzhip_lzma_resume_host(src, n, buf, cap, st, sto, model, ol, iu)


def test_windowed_entry_points(gpu):
    """30 programs -- the expensive packets and the chunk families among them -- through mzhip_lzma_host and mzhip_xz_host,
    and window by window through mzhip_lzma_resume_host (method 14) and mzhip_lzma2_run_host (LZMA2) with the drivers of
    tests/test_kernel_emul.py"""
    from tests.test_kernel_emul import _lzma2_windows, _lzma_windows

    L = gpu.mz.lib()
    H = _HostAsEmul(L)
    for fn in (L.mzhip_lzma_host, L.mzhip_xz_host):
        fn.restype = C.c_int32
        fn.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64] + [C.POINTER(C.c_uint32)] * 3

    def host(fn, z, cap):
        out = C.create_string_buffer(cap + 8)
        ol, iu, crc = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = fn(z, len(z), out, cap, -1, C.byref(ol), C.byref(iu), C.byref(crc))
        return st, iu.value, out.raw[:ol.value], crc.value

    acc = dict((p.name, (p, d)) for p, d in K.accepted())
    pick = [n for n in acc if n.startswith("expensive")] + ["states/edges/pb2", "states/leave/pb4", "reps/queue", "literals/lc0lp4", "literals/lc4lp0",
                                                            "slots/rot5", "window/len512+255/eos2", "dictionary/4100/at/rep3", "overlap/dist1-2"]
    calls = 0
    for name in pick:
        p, want = acc[name]
        z = p.zip14()
        assert host(L.mzhip_lzma_host, z, len(want)) == (0, len(z), want, zlib.crc32(want)), name
        window, gulp = (65536, 300) if name.startswith("expensive") else (4096 if len(want) < 30000 else 65536, 700)
        got, used, rc = _lzma_windows(H, z, len(want), window, gulp, K.round_dict(p.dict_size))
        assert (rc, used) == (0, len(z)) and got == want, (name, rc, used, len(z), len(got), len(want))
        calls += 1
    chunks = dict((p.name, p) for p in K.chunk_programs())
    pick2 = ["chunks/sequence/0", "chunks/sequence/1", "chunks/props/lc0lp4pb2", "chunks/props/lc4lp0pb4", "chunks/dict-reset/e0/after37/first-byte",
             "chunks/dict-reset/01/after37/first-byte", "chunks/raw-between/mlit/raw2", "chunks/raw-between/shortrep/raw1", "chunks/raw-between/rep0/raw50",
             "chunks/raw-between/rep3/raw2", "chunks/usize1", "chunks/csize-max", "chunks/ctl/second/a1", "chunks/ctl/first/e0",
             "chunks/dict-reset/e0/after37/beyond", "chunks/refused/match-crosses-end", "chunks/refused/csize+1"]
    for i, name in enumerate(pick2):
        p = chunks[name]
        want, verdict = p.expand()
        want = bytes(want)
        ok = verdict is None or verdict[0] == "end"
        x = p.xz(CHECKS[i % 4])
        a = host(L.mzhip_xz_host, x, len(want) + 16)
        got, used, rc, cv, _ = _lzma2_windows(H, p.raw(), 4096 if len(want) < 30000 else 65536, 700, p.dict_size, 4)
        if ok:
            assert a == (0, len(x), want, zlib.crc32(want)), (name, a[0], a[1])
            assert (rc, used) == (0, len(p.raw())) and got == want and cv == oracle.crc64(want), (name, rc, used)
        else:
            assert a[0] == -3 and rc == -3, (name, a[0], rc)
        calls += 1
    print("test_windowed_entry_points: %d programs" % calls)
    assert calls <= 30 and sum(n.startswith("expensive") for n in pick) >= 4
