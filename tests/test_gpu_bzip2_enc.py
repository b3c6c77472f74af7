"""GPU tests of the bzip2 encoder (ZIP method 12, the write side): the inputs of tests/bzip2_enc_cases.py through
mzhip_bzip2_encode_batch, judged by libbz2 (Python's bz2) and -- byte for byte -- by the host build of the same header
(bzip2_enc_core.h under -DMZHIP_HOST_EMUL); the input unchanged, nothing outside an entry's region written, result elements
behind n untouched (tests/gpu_util.py); then the capacity status, wave reuse, the launch geometry, mzhip_bzip2_encode_host and
encode_archive(method=12), read back by Python's zipfile and by DeviceArchive.decode."""
import bz2
import ctypes as C
import io
import struct
import zipfile
import zlib
from importlib import import_module

import numpy as np
import pytest

from tests import bzip2_blocks as bb
from tests import bzip2_enc_cases as cs
from tests import gpu_util

pytestmark = pytest.mark.gpu
PW = b"test123"
GUARD = 64
OUT_FULL, PARAM_ERROR = -200, -102


@pytest.fixture(scope="module")
def gpu():
    import torch

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    return gpu_util


def launch(datas, caps, level, packed=False, odd=False, seed=5, max_in_len=None):
    """entries through ONE mzhip_bzip2_encode_batch call, handed over in a shuffled order, inside a seeded pattern with red
    zones (packed: back to back, so every input and output alignment occurs).  check_guards holds the memory contract.
    -> (status, out_len, crc, list of output bytes), in the order of `datas`"""
    import torch

    L = gpu_util.mz.lib()
    n = len(datas)
    b = gpu_util.make_batch(datas, caps, guard=GUARD, fill=seed, packed=packed, odd=odd)
    idx = np.random.RandomState(seed).permutation(n)
    t_idx = torch.from_numpy(idx).cuda()
    d_in_off, d_in_len = b["in_off"][t_idx].contiguous(), b["in_len"][t_idx].contiguous()
    d_out_off, d_cap = b["out_off"][t_idx].contiguous(), b["out_cap"][t_idx].contiguous()
    res = gpu_util.guarded_results(n, ["out_len", "crc", "status"])
    rc = L.mzhip_bzip2_encode_batch(b["d_in"].data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(),
                                    max(len(d) for d in datas) if max_in_len is None else max_in_len, b["d_out"].data_ptr(),
                                    d_out_off.data_ptr(), d_cap.data_ptr(), n, level, res["out_len"].data_ptr(),
                                    res["crc"].data_ptr(), res["status"].data_ptr(), None)
    assert rc == 0, (rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    status, out_len, crc = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status[idx] = res["status"].cpu().numpy()[:n]
    out_len[idx] = gpu_util.result_words(res["out_len"], n)
    crc[idx] = gpu_util.result_words(res["crc"], n)
    assert (out_len <= np.asarray(caps)).all()
    h_out = gpu_util.check_guards(b, out_len, status, res)
    outs = [gpu_util.entry_bytes(b, h_out, i, int(out_len[i])) for i in range(n)]
    for i in range(n):
        assert crc[i] == zlib.crc32(datas[i]), i
    return status, out_len, crc, outs


def by_level(cases):
    out = {}
    for c in cases:
        out.setdefault(c[2], []).append(c)
    return sorted(out.items())


@pytest.mark.parametrize("layout", ["red_zones_odd", "packed"])
def test_cases_equal_the_emulation(gpu, layout):
    """every input of at most 150 000 bytes, one call per level: status 0, libbz2 returns the input, the CRC is the input's,
    and the bytes are the host build's"""
    bound = gpu.mz.lib().mzhip_bzip2_encode_bound
    want = cs.emul_streams()
    for level, cases in by_level([c for c in cs.cases() if len(c[1]) <= 150000]):
        datas = [c[1] for c in cases]
        caps = [int(bound(len(d), level)) for d in datas]
        status, out_len, crc, outs = launch(datas, caps, level, packed=layout == "packed", odd=layout != "packed", seed=5 + level)
        for (name, data, _), st, z in zip(cases, status, outs):
            assert st == 0, (name, st)
            assert bz2.decompress(z) == data, name
            assert z == want[name], (name, "device bytes differ from the emulation's")


def test_out_cap_one_short(gpu):
    """every second entry gets one byte less than it needs: -200 and out_len 0 for it, its neighbours are what they were"""
    want = cs.emul_streams()
    cases = [c for c in cs.cases() if c[2] == 9 and len(c[1]) <= 70000]
    datas = [c[1] for c in cases]
    caps = [len(want[c[0]]) - (i & 1) for i, c in enumerate(cases)]
    status, out_len, crc, outs = launch(datas, caps, 9, packed=True, seed=21)
    for i, (name, data, _) in enumerate(cases):
        if i & 1:
            assert status[i] == OUT_FULL and out_len[i] == 0, (name, status[i])
        else:
            assert status[i] == 0 and outs[i] == want[name], name
    status, out_len, _, _ = launch([b"", b"abc"], [0, 13], 9, seed=22)
    assert list(status) == [OUT_FULL, OUT_FULL] and list(out_len) == [0, 0]


def test_every_wave_reused(gpu):
    """n = 4 x the resident grid, small mixed entries: every wave takes several entries, each kind behind other kinds"""
    L = gpu.mz.lib()
    g, sb = C.c_uint32(0), C.c_uint64(0)
    L.mzhip_bzip2_encode_launch_geometry(0x7FFFFFFF, 700, 9, C.byref(g), C.byref(sb))
    assert g.value > 0
    want = cs.emul_streams()
    small = [c for c in cs.small() if c[2] == 9]
    assert len(small) >= 40
    n = 4 * g.value
    picked = [small[(7 * i) % len(small)] for i in range(n)]
    datas = [c[1] for c in picked]
    status, out_len, crc, outs = launch(datas, [int(L.mzhip_bzip2_encode_bound(len(d), 9)) for d in datas], 9, packed=True, seed=8)
    assert (status == 0).all()
    for (name, data, _), z in zip(picked, outs):
        assert z == want[name], name


def test_launch_geometry(gpu):
    L = gpu.mz.lib()
    g, sb = C.c_uint32(9), C.c_uint64(9)

    def geometry(n, max_in_len, level):
        L.mzhip_bzip2_encode_launch_geometry(n, max_in_len, level, C.byref(g), C.byref(sb))
        return g.value, sb.value

    assert geometry(0, 65536, 9) == (0, 0)
    assert geometry(3, 65536, 7) == (0 + 3, 3 * geometry(1, 65536, 7)[1])
    per_wave_64k, per_wave_900k = geometry(1, 65536, 9)[1], geometry(1, 900000, 9)[1]
    assert per_wave_64k == (17 * 81984 + 18048 + 255) // 256 * 256 and per_wave_900k == (17 * 900032 + 18048 + 255) // 256 * 256
    assert per_wave_64k < per_wave_900k == geometry(1, 1 << 30, 9)[1]
    grid, total = geometry(0x7FFFFFFF, 65536, 9)
    assert total == grid * per_wave_64k
    assert geometry(5, 65536, 0) == (0, 0) and geometry(5, 65536, 10) == (0, 0)
    assert geometry(5, 65536, -1) == geometry(5, 65536, 6)
    # a level that is none: -102, and nothing is launched (the result words keep their fill)
    res = gpu_util.guarded_results(1, ["out_len", "crc", "status"])
    b = gpu_util.make_batch([b"abc"], [64], guard=GUARD, fill=3)
    for level in (0, 10, -2):
        rc = L.mzhip_bzip2_encode_batch(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), 3, b["d_out"].data_ptr(),
                                        b["out_off"].data_ptr(), b["out_cap"].data_ptr(), 1, level, res["out_len"].data_ptr(),
                                        res["crc"].data_ptr(), res["status"].data_ptr(), None)
        assert rc == PARAM_ERROR
        assert L.mzhip_bzip2_encode_bound(100, level) == 0
    import torch
    torch.cuda.synchronize()
    assert (gpu_util.result_words(res["status"], 1) == gpu_util.SENTINEL).all()
    assert (b["d_out"].cpu().numpy() == b["h_fill"]).all()
    assert L.mzhip_bzip2_encode_batch(None, None, None, 0, None, None, None, 0, 9, None, None, None, None) == 0


def test_host_entry_point(gpu):
    T = bb._text(70000, seed=9)
    for k, n in enumerate((0, 1, 15, 16, 17, 63, 64, 65, 70000)):
        level = (1, 9, -1)[k % 3]
        st, z, crc = gpu.mz.bzip2_encode_host(T[:n], level)
        assert st == 0 and crc == zlib.crc32(T[:n]), n
        d = bz2.BZ2Decompressor()
        assert d.decompress(z) == T[:n] and d.eof and d.unused_data == b"" and z[:4] == b"BZh%d" % (6 if level == -1 else level), n
    L = gpu.mz.lib()
    st, z, _ = gpu.mz.bzip2_encode_host(T[:300], 9)
    out = C.create_string_buffer(len(z) + 8)
    ol, crc = C.c_uint32(7), C.c_uint32(0)
    assert L.mzhip_bzip2_encode_host(T[:300], 300, 9, out, len(z) - 1, C.byref(ol), C.byref(crc)) == OUT_FULL and ol.value == 0
    assert out.raw == b"\0" * len(out.raw)
    assert L.mzhip_bzip2_encode_host(T[:300], 300, 9, out, len(z), C.byref(ol), C.byref(crc)) == 0 and out.raw[:ol.value] == z
    assert L.mzhip_bzip2_encode_host(T[:300], 300, 12, out, len(z), C.byref(ol), C.byref(crc)) == PARAM_ERROR


# ---- archives ------------------------------------------------------------------------------------------------------------

def _entries():
    rs = np.random.RandomState(14)
    T = bb._text(30000, seed=6)
    return [("empty.bin", b""), ("text.txt", T), ("noise.bin", rs.bytes(3000)), ("runs.bin", b"\0" * 5000 + b"ab" * 50 + b"\xff" * 300),
            ("one.bin", b"z"), ("text2.txt", T[100:4000])]


def _headers(z, n):
    """(version needed, flag, method, crc, csize, usize, extra) of every local header and directory record"""
    loc, cd, p = [], [], 0
    for _ in range(n):
        p = z.index(b"PK\x03\x04", p)
        need, flag, method, _, _, crc, csize, usize, fn, ex = struct.unpack("<HHHHHIIIHH", z[p + 4:p + 30])
        loc.append((need, flag, method, crc, csize, usize, z[p + 30 + fn:p + 30 + fn + ex]))
        p += 30 + fn + ex + csize
    for _ in range(n):
        p = z.index(b"PK\x01\x02", p)
        _, need, flag, method, _, _, crc, csize, usize, fn, ex = struct.unpack("<HHHHHHIIIHH", z[p + 4:p + 32])
        cd.append((need, flag, method, crc, csize, usize, z[p + 46 + fn:p + 46 + fn + ex]))
        p += 46 + fn + ex
    return loc, cd


def _decode_back(tmp_path, z, ents, password=None):
    path = str(tmp_path / "a.zip")
    with open(path, "wb") as f:
        f.write(z)
    a = import_module("minizip-ng_amd.archive").DeviceArchive(path)
    r = a.decode(password=password)
    assert list(r["status"]) == [0] * len(ents) and r["ok"].all()
    out = r["out"].cpu().numpy()
    for i, (name, data) in enumerate(ents):
        o = int(r["out_off"][i])
        assert int(r["out_len"][i]) == len(data) and out[o:o + len(data)].tobytes() == data, name
        if password is None:
            assert int(r["crc"][i]) == zlib.crc32(data), name
    return a


@pytest.mark.parametrize("kind,ae_version", [(None, 2), ("pk", 2), ("aes", 1), ("aes", 2)])
def test_encode_archive_method_12(gpu, tmp_path, kind, ae_version):
    arch = import_module("minizip-ng_amd.archive")
    ents = _entries()
    z = arch.encode_archive(ents, method=12, level=(9 if kind is None else -1), password=None if kind is None else PW, kind=kind,
                            strength=2, ae_version=ae_version, entropy=lambda k: (bytes(range(1, 256)) * (k // 255 + 1))[:k])
    loc, cd = _headers(z, len(ents))
    assert loc == cd
    over = arch.crypt_overhead(kind, 2)
    for (name, data), (need, flag, method, crc, csize, usize, extra) in zip(ents, loc):
        assert usize == len(data) and flag == (1 if kind else 0), name
        if kind == "aes":
            assert (need, method) == (51, 99) and extra == struct.pack("<HHH2sBH", 0x9901, 7, ae_version, b"AE", 2, 12), name
            assert crc == (0 if ae_version == 2 else zlib.crc32(data)), name
        else:
            assert (need, method, extra, crc) == (46, 12, b"", zlib.crc32(data)), name
        assert csize >= 14 + over
    if kind != "aes":   # Python's zipfile reads plain and ZipCrypto archives
        with zipfile.ZipFile(io.BytesIO(z)) as zf:
            zf.setpassword(PW if kind else None)
            assert zf.testzip() is None
            for (name, data), zi in zip(ents, zf.infolist()):
                assert zi.compress_type == zipfile.ZIP_BZIP2 and zf.read(zi) == data, name
    a = _decode_back(tmp_path, z, ents, password=None if kind is None else PW)
    assert [int(m) for m in a.table[:, 0]] == [99 if kind == "aes" else 12] * len(ents)


def test_encode_archive_still_refuses(gpu):
    arch = import_module("minizip-ng_amd.archive")
    for method in (95, 93, 1):
        with pytest.raises(gpu.mz.MzHipError):
            arch.encode_archive([("a", b"abc")], method=method)
    with pytest.raises(gpu.mz.MzHipError):
        arch.encode_archive([("a", b"abc")], method=12, level=0)
    assert arch.encode_archive([], method=12)[:4] == b"PK\x05\x06"
