"""GPU tests of the Zstandard encoder (ZIP method 93, the write side): the inputs of tests/zstd_enc_cases.py through
mzhip_zstd_encode_batch, judged -- byte for byte -- by the host build of the same header (zstd_enc_core.h under
-DMZHIP_HOST_EMUL) and read back by the device's own decoder (mzhip_zstd_batch); the input unchanged, nothing outside an
entry's region written, result elements behind n untouched (tests/gpu_util.py); then the capacity status, wave reuse, the
launch geometry, mzhip_zstd_encode_host and encode_zstd_archive, read back by DeviceArchive.decode.  No test needs libzstd."""
import ctypes as C
import struct
import zlib
from importlib import import_module

import numpy as np
import pytest

from tests import gpu_util
from tests import synth
from tests import zstd_enc_cases as cs
from tests import zstd_frames as zf
from tests import zstd_tokens as zt

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


def launch(datas, caps, level, flags=0, packed=False, odd=False, seed=5, max_in_len=None):
    """entries through ONE mzhip_zstd_encode_batch call, handed over in a shuffled order, inside a seeded pattern with red
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
    rc = L.mzhip_zstd_encode_batch(b["d_in"].data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(),
                                   max(len(d) for d in datas) if max_in_len is None else max_in_len, b["d_out"].data_ptr(),
                                   d_out_off.data_ptr(), d_cap.data_ptr(), n, level, flags, res["out_len"].data_ptr(),
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


def decode_back(frames, datas):
    """the frames through mzhip_zstd_batch: status 0, the input's bytes and CRC"""
    import torch

    caps = [max(len(d), 1) for d in datas]
    b = gpu_util.make_batch(frames, caps, guard=GUARD, fill=77)
    out_len, in_used, crc, status = gpu_util.mz.zstd_batch(b["d_in"], b["in_off"], b["in_len"], b["d_out"], b["out_off"], b["out_cap"])
    torch.cuda.synchronize()
    h_out = b["d_out"].cpu().numpy()
    st, ol = status.cpu().numpy(), gpu_util.mz.u32(out_len)
    for i, d in enumerate(datas):
        assert st[i] == 0 and int(ol[i]) == len(d), (i, st[i])
        assert gpu_util.entry_bytes(b, h_out, i, len(d)) == d, i
    assert list(gpu_util.mz.u32(crc)) == [zlib.crc32(d) for d in datas]


def by_class(cases):
    out = {}
    for c in cases:
        out.setdefault((c[2], c[3]), []).append(c)
    return sorted(out.items())


@pytest.mark.parametrize("layout", ["red_zones_odd", "packed"])
def test_cases_equal_the_emulation(gpu, layout):
    """every input, one call per level and flag word: status 0, the CRC is the input's, the bytes are the host build's, and the
    device's decoder returns the input"""
    bound = gpu.mz.lib().mzhip_zstd_encode_bound
    want = cs.emul_streams()
    for (level, flags), cases in by_class(cs.cases()):
        datas = [c[1] for c in cases]
        caps = [int(bound(len(d))) for d in datas]
        status, out_len, crc, outs = launch(datas, caps, level, flags, packed=layout == "packed", odd=layout != "packed", seed=5 + level + flags)
        for (name, data, _, _), st, z in zip(cases, status, outs):
            assert st == 0, (name, st)
            assert z == want[name], (name, "device bytes differ from the emulation's")
        if layout == "packed":
            decode_back(outs, datas)


def test_window_descriptor_path(gpu):
    """one entry of 8 MiB + 70 000 bytes: a Window_Descriptor of 8 MiB, a 4-byte content size, the checksum; the device's decoder
    returns the input"""
    name, data, level, flags = cs.big()
    status, out_len, crc, outs = launch([data], [int(gpu.mz.lib().mzhip_zstd_encode_bound(len(data)))], level, flags, seed=31)
    z = outs[0]
    assert status[0] == 0 and z[4] == 0x84 and z[5] == 0x68 and int.from_bytes(z[6:10], "little") == len(data)
    assert int.from_bytes(z[-4:], "little") == zf.xxh64(data) & 0xFFFFFFFF and len(z) < len(data) // 2
    decode_back([z], [data])


def test_out_cap_one_short(gpu):
    """every second entry gets one byte less than it needs: -200 and out_len 0 for it, its neighbours are what they were"""
    want = cs.emul_streams()
    cases = [c for c in cs.cases() if (c[2], c[3]) == (3, 0) and len(c[1]) <= 70000]
    datas = [c[1] for c in cases]
    caps = [len(want[c[0]]) - (i & 1) for i, c in enumerate(cases)]
    status, out_len, crc, outs = launch(datas, caps, 3, packed=True, seed=21)
    for i, (name, data, _, _) in enumerate(cases):
        if i & 1:
            assert status[i] == OUT_FULL and out_len[i] == 0, (name, status[i])
        else:
            assert status[i] == 0 and outs[i] == want[name], name
    status, out_len, _, _ = launch([b"", b"abc"], [0, 11], 3, seed=22)
    assert list(status) == [OUT_FULL, OUT_FULL] and list(out_len) == [0, 0]


def test_every_wave_reused(gpu):
    """n = 4 x the resident grid, small mixed entries: every wave takes several entries; a Raw-block entry sits behind a
    compressed one and the other way round"""
    L = gpu.mz.lib()
    g, sb = C.c_uint32(0), C.c_uint64(0)
    L.mzhip_zstd_encode_launch_geometry(0x7FFFFFFF, 700, 3, C.byref(g), C.byref(sb))
    assert g.value > 0
    want = cs.emul_streams()
    small = [c for c in cs.small() if (c[2], c[3]) == (3, 0)] + [c for c in cs.cases() if c[0] in ("noise_1000", "streams_1023", "nseq_128")]
    kinds = set(zt.read(want[c[0]])[0]["blocks"][0]["type"] for c in small)
    assert {"raw", "compressed"} <= kinds
    n = 4 * g.value
    picked = [small[(5 * i) % len(small)] for i in range(n)]
    datas = [c[1] for c in picked]
    status, out_len, crc, outs = launch(datas, [int(L.mzhip_zstd_encode_bound(len(d))) for d in datas], 3, packed=True, seed=8)
    assert (status == 0).all()
    for (name, data, _, _), z in zip(picked, outs):
        assert z == want[name], name


def test_launch_geometry(gpu):
    L = gpu.mz.lib()
    g, sb = C.c_uint32(9), C.c_uint64(9)

    def geometry(n, max_in_len, level):
        L.mzhip_zstd_encode_launch_geometry(n, max_in_len, level, C.byref(g), C.byref(sb))
        return g.value, sb.value

    per_wave = 65536 + 8 * 16384 + 65536 + 1024

    def expect(n, blocks, grid):        # tokens, token counts, three counters (rounded up to 256), the coder's part per wave
        words = n * blocks * 65536
        if blocks > 1:
            words += n * blocks * 65536 + (min(n, 1024) << 18)
        return (4 * (words + n * blocks + 3) + 255) // 256 * 256 + grid * per_wave

    assert geometry(0, 65536, 3) == (0, 0)
    assert geometry(3, 65536, 3) == (3, expect(3, 1, 3)) and geometry(3, 0, 3) == (3, expect(3, 1, 3))
    assert geometry(2, 65537, 1) == (2, expect(2, 2, 2)) and geometry(1, 1 << 20, 19) == (1, expect(1, 16, 1))
    grid, total = geometry(100000, 700, 3)
    assert 0 < grid < 100000 and total == expect(100000, 1, grid)
    assert geometry(5, 65536, 23) == (0, 0) and geometry(5, 65536, -2) == (0, 0)
    assert geometry(5, 65536, -1) == geometry(5, 65536, 3) == geometry(5, 65536, 0)
    assert [L.mzhip_zstd_encode_bound(k) for k in (0, 1, 65536, 65537)] == [17, 18, 65536 + 17, 65537 + 20]
    # a level that is none: -102, and nothing is launched (the result words keep their fill)
    res = gpu_util.guarded_results(1, ["out_len", "crc", "status"])
    b = gpu_util.make_batch([b"abc"], [64], guard=GUARD, fill=3)
    for level in (23, -2, 100):
        rc = L.mzhip_zstd_encode_batch(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), 3, b["d_out"].data_ptr(),
                                       b["out_off"].data_ptr(), b["out_cap"].data_ptr(), 1, level, 0, res["out_len"].data_ptr(),
                                       res["crc"].data_ptr(), res["status"].data_ptr(), None)
        assert rc == PARAM_ERROR
    import torch
    torch.cuda.synchronize()
    assert (gpu_util.result_words(res["status"], 1) == gpu_util.SENTINEL).all()
    assert (b["d_out"].cpu().numpy() == b["h_fill"]).all()
    assert L.mzhip_zstd_encode_batch(None, None, None, 0, None, None, None, 0, 3, 0, None, None, None, None) == 0


def test_host_entry_point(gpu):
    T = synth.corpus()[5000:75000]
    w = cs.load_emul().emul_zstd_enc_wave_new()
    for k, n in enumerate((0, 1, 15, 16, 17, 63, 64, 65, 70000)):
        level, checksum = (1, 3, -1, 19)[k % 4], bool(k & 1)
        st, z, crc = gpu.mz.zstd_encode_host(T[:n], level, checksum)
        assert st == 0 and crc == zlib.crc32(T[:n]), n
        assert z == cs.emul_encode(w, T[:n], level, int(checksum))[1], n
        assert zf.expand(z) == (0, T[:n], len(z)), n
    cs.load_emul().emul_zstd_enc_wave_free(w)
    L = gpu.mz.lib()
    st, z, _ = gpu.mz.zstd_encode_host(T[:300], 3)
    out = C.create_string_buffer(len(z) + 8)
    ol, crc = C.c_uint32(7), C.c_uint32(0)
    assert L.mzhip_zstd_encode_host(T[:300], 300, 3, 0, out, len(z) - 1, C.byref(ol), C.byref(crc)) == OUT_FULL and ol.value == 0
    assert out.raw == b"\0" * len(out.raw)
    assert L.mzhip_zstd_encode_host(T[:300], 300, 3, 0, out, len(z), C.byref(ol), C.byref(crc)) == 0 and out.raw[:ol.value] == z
    for level in (23, -2):
        assert L.mzhip_zstd_encode_host(T[:300], 300, level, 0, out, len(z), C.byref(ol), C.byref(crc)) == PARAM_ERROR


# ---- archives ------------------------------------------------------------------------------------------------------------

def _entries():
    rs = np.random.RandomState(14)
    T = synth.corpus()[:30000]
    return [("empty.bin", b""), ("text.txt", T), ("noise.bin", rs.bytes(3000)), ("runs.bin", b"\0" * 5000 + b"ab" * 50 + b"\xff" * 300),
            ("one.bin", b"z"), ("text2.txt", T[100:4000]), ("two_blocks.txt", synth.corpus()[40000:40000 + 70000])]


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
def test_encode_zstd_archive(gpu, tmp_path, kind, ae_version):
    arch = import_module("minizip-ng_amd.archive")
    ents = _entries()
    checksum = kind is None
    z = arch.encode_zstd_archive(ents, level=(19 if kind is None else -1), checksum=checksum, password=None if kind is None else PW, kind=kind,
                                 strength=2, ae_version=ae_version, entropy=lambda k: (bytes(range(1, 256)) * (k // 255 + 1))[:k])
    loc, cd = _headers(z, len(ents))
    assert loc == cd
    over = arch.crypt_overhead(kind, 2)
    for (name, data), (need, flag, method, crc, csize, usize, extra) in zip(ents, loc):
        assert usize == len(data) and flag == (1 if kind else 0), name
        if kind == "aes":
            assert (need, method) == (51, 99) and extra == struct.pack("<HHH2sBH", 0x9901, 7, ae_version, b"AE", 2, 93), name
            assert crc == (0 if ae_version == 2 else zlib.crc32(data)), name
        else:
            assert (need, method, extra, crc) == (20, 93, b"", zlib.crc32(data)), name
        assert csize >= 9 + over
    if kind is None:      # the payloads are the frames: the plain reader takes them, checksum and all
        p = 0
        for (name, data), (_, _, _, _, csize, _, _) in zip(ents, loc):
            p = z.index(b"PK\x03\x04", p)
            fn = struct.unpack("<H", z[p + 26:p + 28])[0]
            frame = z[p + 30 + fn:p + 30 + fn + csize]
            assert zf.expand(frame) == (0, data, csize) and zt.read(frame)[0]["checksum"], name
            p += 30 + fn + csize
    a = _decode_back(tmp_path, z, ents, password=None if kind is None else PW)
    assert [int(m) for m in a.table[:, 0]] == [99 if kind == "aes" else 93] * len(ents)


def test_archive_levels_refused_and_names(gpu):
    arch = import_module("minizip-ng_amd.archive")
    for level in (23, -2):
        with pytest.raises(gpu.mz.MzHipError):
            arch.encode_zstd_archive([("a", b"abc")], level=level)
    with pytest.raises(gpu.mz.MzHipError):
        arch.encode_archive([("a", b"abc")], method=93)          # the old door stays shut: encode_zstd_archive is the new one
    with pytest.raises(gpu.mz.MzHipError):
        arch.assemble_archive(["a"], [b"abc"], [0], [3], method=95)
    assert arch.encode_zstd_archive([])[:4] == b"PK\x05\x06"
    z = arch.assemble_archive(["a"], [b"abc"], [0], [3], method=93)
    assert struct.unpack("<HHH", z[4:10]) == (20, 0, 93)
