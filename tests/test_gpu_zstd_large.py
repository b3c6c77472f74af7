"""GPU tests of mzhip_zstd_large (one large method-93 entry, a wave per Zstandard block): the multi-block programs of
tests/zstd_large_cases.py at the default window and at windows of 4096 bytes against mzhip_zstd_batch on the same entry and
against the host build of the same passes -- every field, and the counters; the project's own encoder read back; capacity one
short; guard bytes around input and output; DeviceArchive.decode routing large method-93 entries through it, plain and behind
AES, with the same results in every field.  No test here needs libzstd."""
import ctypes as C
import zlib
from importlib import import_module

import numpy as np
import pytest

from tests import crypt_ref as cr
from tests import gpu_util
from tests import synth
from tests import zstd_frames as zf
from tests import zstd_large_cases as zc
from tests.test_gpu_zstd import PW, _archive, _bytes_of, _mixed, _write
from tests.test_zstd_large_emul import build_emul, run as emul_run

pytestmark = pytest.mark.gpu
GUARD = 64
COUNTERS = ("windows", "blocks", "borrowed", "fallback")     # (rounds: how far a racing lane sees depends on the schedule)


@pytest.fixture(scope="module")
def gpu():
    import torch

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    return gpu_util


def batch_reference(b):
    """mzhip_zstd_batch over a batch -> (status, out_len, in_used, crc, host copy of d_out)"""
    import torch

    out_len, in_used, crc, status = gpu_util.mz.zstd_batch(b["d_in"], b["in_off"], b["in_len"], b["d_out"], b["out_off"], b["out_cap"])
    torch.cuda.synchronize()
    return status.cpu().numpy(), gpu_util.mz.u32(out_len), gpu_util.mz.u32(in_used), gpu_util.mz.u32(crc), b["d_out"].cpu().numpy()


def large_each(b, window):
    """every entry of a batch through its own mzhip_zstd_large call, where it lies -> (status, out_len, in_used, crc, stats)"""
    L = gpu_util.mz.lib()
    n = b["n"]
    status, out_len, in_used, crc, stats = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), []
    for i in range(n):
        ol, iu, ck, st = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_uint32(0x12345678), C.c_int32(77)
        s = gpu_util.mz.ZstdLargeStats(size=C.sizeof(gpu_util.mz.ZstdLargeStats))
        rc = L.mzhip_zstd_large(b["d_in"].data_ptr() + int(b["h_in_off"][i]), int(b["h_in_len"][i]), b["d_out"].data_ptr() + int(b["h_out_off"][i]),
                                int(b["h_out_cap"][i]), window, C.byref(ol), C.byref(iu), C.byref(ck), C.byref(st), C.byref(s), None)
        assert rc == 0, (i, rc, L.mzhip_last_error())
        status[i], out_len[i], in_used[i], crc[i] = st.value, ol.value, iu.value, ck.value
        stats.append(dict((k, int(getattr(s, k))) for k in COUNTERS + ("rounds",)))
    return status, out_len, in_used, crc, stats


def parity(cases, caps, window, emu=None, seed=5, **layout):
    """the entries through mzhip_zstd_batch and, in a second batch of the same layout, through mzhip_zstd_large: every field
    and every byte equal, the memory contract kept (tests/gpu_util.py check_guards); with emu, the emulation's fields and counters too"""
    zs = [c[1] for c in cases]
    ref = batch_reference(gpu_util.make_batch(zs, caps, guard=GUARD, fill=seed, **layout))
    b = gpu_util.make_batch(zs, caps, guard=GUARD, fill=seed, **layout)
    status, out_len, in_used, crc, stats = large_each(b, window)
    h_out = gpu_util.check_guards(b, out_len, status)
    for i, c in enumerate(cases):
        assert (status[i], out_len[i], in_used[i], crc[i]) == (ref[0][i], ref[1][i], ref[2][i], ref[3][i]), (c[0], window)
        got = gpu_util.entry_bytes(b, h_out, i, int(out_len[i]))
        assert got == gpu_util.entry_bytes(b, ref[4], i, int(out_len[i])) and crc[i] == zlib.crc32(got), c[0]
        if emu is not None:
            e, es = emul_run(emu, c[1], caps[i], window=window, seed=i + 1)
            assert (status[i], out_len[i], in_used[i], got, crc[i]) == e, c[0]
            assert [stats[i][k] for k in COUNTERS] == [es[k] for k in COUNTERS], (c[0], stats[i], es)
            assert (stats[i]["rounds"] > 0) == (es["rounds"] > 0), c[0]
    return status, out_len, stats


@pytest.mark.parametrize("window", [0, 4096])
def test_case_parity(gpu, window):
    cases = zc.cases()
    caps = [len(c[3]) if c[2] == 0 else 4096 for c in cases]
    status, out_len, stats = parity(cases, caps, window, emu=build_emul(), odd=True)
    for i, (name, z, st, data, used, blocks, borrowed) in enumerate(cases):
        if st != 0:
            st, data, used = zf.expand(z, caps[i])
        assert status[i] == st and out_len[i] == len(data), name
        if zc.over_cap(name):
            assert stats[i]["fallback"] == 2, name
        elif st == 0:
            assert (stats[i]["fallback"], stats[i]["blocks"], stats[i]["borrowed"]) == (0, blocks, borrowed), (name, stats[i])
        else:
            assert stats[i]["fallback"] == 1, name


def test_programs_of_zstd_frames_packed(gpu):
    """the one-block families back to back, so every input and output alignment occurs"""
    cases = [v for v in zf.verdicts() if len(v[1]) < 3000 and len(v[3]) < 3000][::3] + [(n, z, 0, d, len(z)) for n, z, d in zf.payloads()]
    caps = [len(c[3]) if c[2] == 0 else 4096 for c in cases]
    status, _, stats = parity(cases, caps, 4096, packed=True)
    for i, c in enumerate(cases):
        assert (stats[i]["fallback"] == 0) == (c[2] == 0) == (status[i] == 0), c[0]


@pytest.mark.parametrize("checksum", [False, True])
def test_own_encoder_round_trip(gpu, checksum):
    """1 MiB + 1 byte of the corpus written by mzhip_zstd_encode_batch (17 blocks) and read back by a wave per block"""
    import torch

    text = synth.corpus()
    d = (text * ((1 << 20) // len(text) + 2))[:(1 << 20) + 1]
    st, z, _ = gpu_util.mz.zstd_encode_host(d, 3, checksum)
    assert st == 0 and zc.census(z)[0] == 17
    for window in (0, 300000):
        d_in = torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy()).cuda()
        d_out = torch.zeros(len(d), dtype=torch.uint8, device="cuda")
        st, ol, iu, crc, s = gpu_util.mz.zstd_large(d_in, d_out, window)
        assert (st, ol, iu, crc) == (0, len(d), len(z), zlib.crc32(d))
        assert d_out.cpu().numpy().tobytes() == d
        assert s["blocks"] == 17 and s["fallback"] == 0 and s["rounds"] >= 2, s
        assert s["windows"] == 1 if window == 0 else 4 <= s["windows"] <= 17, s      # (at least 1 MiB / 300 000 windows)


def test_out_cap_one_short_and_guards(gpu):
    """out_cap one short gives the one-wave status; room to spare changes nothing; nothing outside the entry's buffers is written"""
    cases = [c for c in zc.cases() if c[2] == 0 and len(c[3]) > 0 and not zc.over_cap(c[0])]
    status, out_len, stats = parity(cases, [len(c[3]) - 1 for c in cases], 4096, odd=True, seed=6)
    for i, c in enumerate(cases):
        want = zf.expand(c[1], len(c[3]) - 1)
        assert (status[i], out_len[i]) == (want[0], len(want[1])) and want[0] == zf.OUT_FULL and stats[i]["fallback"] == 1, c[0]
    status, out_len, stats = parity(cases, [len(c[3]) + 37 for c in cases], 0, packed=True, seed=7)
    assert (status == 0).all() and all(s["fallback"] == 0 for s in stats)
    status, _, _ = parity(cases[:6], [0] * 6, 0, seed=8)
    assert (status == zf.OUT_FULL).all()


def _routed_archive(kind=None):
    """the mixed archive of tests/test_gpu_zstd.py (methods 0 / 8 / 12 / 93) and one zstd entry of 1 MiB of the corpus"""
    text = synth.corpus()
    d = (text * ((1 << 20) // len(text) + 2))[7:(1 << 20) + 7]
    st, z, _ = gpu_util.mz.zstd_encode_host(d, 3, True)
    assert st == 0 and len(z) > (64 << 10)
    ents = _mixed()[:6] + [("zstd_1m.txt", 93, d, z)] + _mixed()[6:]
    if kind == "aes":
        ents = [(name, m, data, cr.wz_encrypt(PW, pay, 2, salt_seed=i + 1)) for i, (name, m, data, pay) in enumerate(ents)]
    return ents


@pytest.mark.parametrize("kind", [None, "aes"])
def test_archive_routing(gpu, tmp_path, monkeypatch, kind):
    """with LARGE_ZSTD_ENTRY at 64 KiB the large method-93 entries go through mzhip_zstd_large: no field of the result differs"""
    arch = import_module("minizip-ng_amd.archive")
    ents = _routed_archive(kind)
    path = str(tmp_path / "routed.zip")
    _write(path, ents, kind=kind, **(dict(strength=2, ae_version=2) if kind else {}))
    pw = PW if kind else None
    L = gpu_util.mz.lib()
    real, calls = L.mzhip_zstd_large, []

    def counted(*a):
        calls.append(int(a[1]))
        return real(*a)
    monkeypatch.setattr(L, "mzhip_zstd_large", counted, raising=False)
    assert arch.LARGE_ZSTD_ENTRY == 4 << 20
    r0 = _archive(path).decode(password=pw)
    assert calls == []
    monkeypatch.setattr(arch, "LARGE_ZSTD_ENTRY", 64 << 10)
    r1 = _archive(path).decode(password=pw)
    assert len(calls) >= 1 and all(n >= (64 << 10) for n in calls)
    assert list(r0["status"]) == [0] * len(ents) and r0["ok"].all()
    for k in ("crc", "out_len", "status", "ok", "out_off"):
        assert (np.asarray(r0[k]) == np.asarray(r1[k])).all(), k
    for i, (name, _, data, _) in enumerate(ents):
        assert _bytes_of(r1, i, len(data)) == data, name


def test_archive_routing_damaged_entry(gpu, tmp_path, monkeypatch):
    """a damaged large entry reports as before: the one-wave reader's status for it, the others untouched"""
    arch = import_module("minizip-ng_amd.archive")
    ents = _routed_archive()
    path = str(tmp_path / "damaged.zip")
    raw = bytearray(_write(path, ents))
    p = raw.index(ents[6][3])
    raw[p + (2 * len(ents[6][3])) // 3] ^= 0x21
    want = zf.expand(bytes(raw[p:p + len(ents[6][3])]), len(ents[6][2]))
    assert want[0] != 0
    with open(path, "wb") as f:
        f.write(raw)
    r0 = _archive(path).decode()
    monkeypatch.setattr(arch, "LARGE_ZSTD_ENTRY", 64 << 10)
    r1 = _archive(path).decode()
    assert int(r1["status"][6]) == want[0] and int(r1["out_len"][6]) == len(want[1]) and int(r1["crc"][6]) == zlib.crc32(want[1])
    for k in ("crc", "out_len", "status", "ok"):
        assert (np.asarray(r0[k]) == np.asarray(r1[k])).all(), k
