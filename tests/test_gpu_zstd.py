"""GPU tests of the Zstandard batch path (ZIP method 93): the program families of tests/zstd_frames.py and libzstd's committed
streams through mzhip_zstd_batch, against the verdicts of expand() -- status, out_len, in_used, bytes and CRC-32 exact per
entry, the input unchanged, nothing outside an entry's region written, result elements behind n untouched
(tests/gpu_util.py) -- and against the host emulation of the same core; then mzhip_zstd_host and DeviceArchive.decode on
archives that hold method-93 entries, plain and encrypted.  No test here needs libzstd."""
import bz2
import ctypes as C
import os
import struct
import zlib
from importlib import import_module

import numpy as np
import pytest

from tests import crypt_ref as cr
from tests import gpu_util
from tests import zstd_frames as zf
from tests.test_zstd_emul import build_emul, run as emul_run

pytestmark = pytest.mark.gpu
PW = b"test123"
GUARD = 64
SCRATCH = 131328
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    import torch

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    return gpu_util


def launch(entries, caps, packed=False, odd=False, seed=5, shuffle=True):
    """entries through ONE mzhip_zstd_batch call, handed over in a shuffled order, inside a seeded pattern with red zones
    (packed: back to back, so every input and output alignment occurs).  check_guards holds the memory contract.
    -> (status, out_len, in_used, crc, list of output bytes), in the order of `entries`"""
    import torch

    L = gpu_util.mz.lib()
    n = len(entries)
    b = gpu_util.make_batch(entries, caps, guard=GUARD, fill=seed, packed=packed, odd=odd)
    idx = np.random.RandomState(seed).permutation(n) if shuffle else np.arange(n)
    t_idx = torch.from_numpy(idx).cuda()
    d_in_off, d_in_len = b["in_off"][t_idx].contiguous(), b["in_len"][t_idx].contiguous()
    d_out_off, d_cap = b["out_off"][t_idx].contiguous(), b["out_cap"][t_idx].contiguous()
    res = gpu_util.guarded_results(n, ["out_len", "in_used", "crc", "status"])
    rc = L.mzhip_zstd_batch(b["d_in"].data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), b["d_out"].data_ptr(),
                            d_out_off.data_ptr(), d_cap.data_ptr(), n, res["out_len"].data_ptr(), res["in_used"].data_ptr(),
                            res["crc"].data_ptr(), res["status"].data_ptr(), None)
    assert rc == 0, (rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    status, out_len, in_used, crc = (np.zeros(n, dtype=np.int64) for _ in range(4))
    status[idx] = res["status"].cpu().numpy()[:n]
    out_len[idx] = gpu_util.result_words(res["out_len"], n)
    in_used[idx] = gpu_util.result_words(res["in_used"], n)
    crc[idx] = gpu_util.result_words(res["crc"], n)
    assert (out_len <= np.asarray(caps)).all() and (in_used <= b["h_in_len"]).all()
    h_out = gpu_util.check_guards(b, out_len, status, res)
    outs = [gpu_util.entry_bytes(b, h_out, i, int(out_len[i])) for i in range(n)]
    for i in range(n):
        assert crc[i] == zlib.crc32(outs[i]), i
    return status, out_len, in_used, crc, outs


def cap_of(c):
    """out_cap: the exact length for valid streams, 4 KiB otherwise"""
    return len(c[3]) if c[2] == 0 else 4096


def check(cases, **kw):
    """cases: (name, stream, status, data, in_used) as expand() reads them; a failing stream is read again with the out_cap it
    gets here, and the bytes of the complete blocks in front of its problem are compared too"""
    caps = [cap_of(c) for c in cases]
    status, out_len, in_used, crc, outs = launch([c[1] for c in cases], caps, **kw)
    for i, (name, z, st, data, used) in enumerate(cases):
        if st != 0:
            st, data, used = zf.expand(z, caps[i])
        assert status[i] == st, (name, status[i], st)
        assert out_len[i] == len(data) and outs[i] == data and crc[i] == zlib.crc32(data), name
        if st == 0:
            assert in_used[i] == used, name


def _payload_cases():
    return [(name, z, 0, d, len(z)) for name, z, d in zf.payloads()]


@pytest.mark.parametrize("layout", ["red_zones_odd", "packed"])
def test_programs_and_compressor_output(gpu, layout):
    check(zf.verdicts() + _payload_cases(), packed=layout == "packed", odd=layout != "packed")


def test_device_equals_the_emulation(gpu):
    """the failing entries too: status, out_len, in_used and crc of the device against the host build of the same header"""
    emu = build_emul()
    w = emu.emul_zstd_wave_new()
    cases = [c for c in zf.verdicts() if len(c[1]) <= 4096 and len(c[3]) <= 4096]
    caps = [max(len(c[3]) - (k % 3 == 2), 0) if c[2] == 0 else 4096 for k, c in enumerate(cases)]
    status, out_len, in_used, crc, outs = launch([c[1] for c in cases], caps, odd=True, seed=11)
    for i, c in enumerate(cases):
        st, ol, iu, got, ck = emul_run(emu, w, c[1], caps[i])
        assert (status[i], out_len[i], in_used[i], crc[i], outs[i]) == (st, ol, iu, ck, got), c[0]
    emu.emul_zstd_wave_free(w)


def test_out_cap_one_less_is_out_full(gpu):
    cases = [c for c in zf.verdicts() + _payload_cases() if c[2] == 0 and 0 < len(c[3]) <= 20000]
    status, out_len, _, _, outs = launch([c[1] for c in cases], [len(c[3]) - 1 for c in cases], odd=True, seed=6)
    assert (status == zf.OUT_FULL).all(), [c[0] for c, s in zip(cases, status) if s != zf.OUT_FULL]
    for c, o in zip(cases, outs):
        assert c[3].startswith(o)
    # the first problem in stream order decides
    T = zf.text(700, 5)
    f = zf.Frame(checksum=True, checksum_xor=1)
    f.content = T
    z = f.raw(T[:300]).comp(T[300:], lit_mode="huf").bytes()
    status, out_len, _, _, _ = launch([z, z, z, z[:-2], b""], [299, 699, 700, 700, 16], seed=7)
    assert list(status) == [zf.OUT_FULL, zf.OUT_FULL, zf.DATA_ERROR, zf.BUF_ERROR, zf.BUF_ERROR] and list(out_len) == [0, 300, 700, 700, 0]


def test_every_wave_reused(gpu):
    """n = 4 x the resident grid, small mixed entries: every wave takes several entries, each kind behind other kinds"""
    g, sb = C.c_uint32(0), C.c_uint64(0)
    gpu.mz.lib().mzhip_zstd_launch_geometry(0x7FFFFFFF, C.byref(g), C.byref(sb))
    assert g.value > 0 and sb.value == g.value * SCRATCH
    small = [c for c in zf.verdicts() + _payload_cases() if len(c[1]) <= 700 and len(c[3]) <= 4096]
    assert len(small) >= 300
    n = 4 * g.value
    check([small[(7 * i) % len(small)] for i in range(n)], packed=True, seed=8)


def test_launch_geometry(gpu):
    g, sb = C.c_uint32(9), C.c_uint64(9)
    gpu.mz.lib().mzhip_zstd_launch_geometry(3, C.byref(g), C.byref(sb))
    assert (g.value, sb.value) == (3, 3 * SCRATCH)
    gpu.mz.lib().mzhip_zstd_launch_geometry(0, C.byref(g), C.byref(sb))
    assert (g.value, sb.value) == (0, 0)


def test_host_entry_point(gpu):
    L = gpu.mz.lib()
    name, z3, d3 = [p for p in zf.payloads() if p[0] == "text_64k_l19"][0]
    damaged = bytearray(z3)
    damaged[len(z3) // 2] ^= 0x10
    for z, cap in ((z3, len(d3)), (z3 + b"behind", len(d3)), (bytes(damaged), len(d3)), (z3[:-3], len(d3)), (z3, len(d3) - 1), (b"", 4)):
        st, data, used = zf.expand(z, cap)
        out = C.create_string_buffer(max(cap, 1) + 8)
        ol, iu, crc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        got = L.mzhip_zstd_host(z, len(z), out, cap, C.byref(ol), C.byref(iu), C.byref(crc))
        assert got == st, (got, st)
        assert out.raw[cap:] == b"\0" * (len(out.raw) - cap)
        assert (ol.value, crc.value) == (len(data), zlib.crc32(data)) and out.raw[:ol.value] == data
        if st == 0:
            assert iu.value == used
    assert gpu.mz.zstd_host(z3, len(d3)) == (0, len(z3), d3, zlib.crc32(d3))


def test_python_batch_wrapper(gpu):
    import torch

    ps = zf.payloads()[:6]
    b = gpu_util.make_batch([p[1] for p in ps], [len(p[2]) for p in ps])
    out_len, in_used, crc, status = gpu.mz.zstd_batch(b["d_in"], b["in_off"], b["in_len"], b["d_out"], b["out_off"], b["out_cap"])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(ps) and out_len.cpu().tolist() == [len(p[2]) for p in ps]
    assert list(gpu.mz.u32(crc)) == [zlib.crc32(p[2]) for p in ps]


# ---- DeviceArchive -------------------------------------------------------------------------------------------------------

def _archive(path):
    return import_module("minizip-ng_amd.archive").DeviceArchive(path)


def _relabel(archive, methods, kind=None):
    """an archive assemble_archive wrote as method 8, relabelled entry by entry: the method field of the local header and the
    directory record (plain, ZipCrypto) or the real-method field of the 0x9901 extra field (AES)"""
    z = bytearray(archive)
    for sig, at in ((b"PK\x03\x04", 8), (b"PK\x01\x02", 10)):
        p = 0
        for m in methods:
            p = z.index(sig, p)
            if kind == "aes":
                q = z.index(b"\x01\x99\x07\x00", p)
                assert z[q + 9:q + 11] == b"\x08\x00"
                z[q + 9:q + 11] = struct.pack("<H", m)
            else:
                assert z[p + at:p + at + 2] == b"\x08\x00"
                z[p + at:p + at + 2] = struct.pack("<H", m)
            p += 4
    return bytes(z)


def _pack(method, data, zstd_stream=None):
    if method == 0:
        return data
    if method == 8:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(data) + c.flush()
    if method == 12:
        return bz2.compress(data)
    return zstd_stream


def _mixed():
    """[(name, method, data, payload)]: zstd payloads are libzstd's committed streams and frames of the writer"""
    P = dict((name, (z, d)) for name, z, d in zf.payloads())
    V = dict((v[0], (v[1], v[3])) for v in zf.verdicts())
    T = zf.text(6000, 41)
    ents = [("stored.txt", 0, T[:900], None), ("deflate.txt", 8, T[:5000], None), ("zstd_64k.txt", 93) + P["text_64k_l3"][::-1],
            ("bzip2.txt", 12, T, None), ("zstd_noise.bin", 93) + P["noise_3k_l3"][::-1], ("zstd_empty", 93) + P["empty_l3"][::-1],
            ("deflate2.txt", 8, T[2000:4000], None), ("zstd_zeros.bin", 93) + P["zeros_70k_l3"][::-1],
            ("zstd_frames.bin", 93) + V["two_frames"][::-1], ("zstd_300k.txt", 93) + P["text_300k_l1"][::-1],
            ("zstd_skippable.bin", 93) + V["skippable_5_n"][::-1]]
    return [(name, m, d, _pack(m, d, z)) for name, m, d, z in ents]


def _write(path, ents, kind=None, **kw):
    arch = import_module("minizip-ng_amd.archive")
    z = arch.assemble_archive([e[0] for e in ents], [e[3] for e in ents], [zlib.crc32(e[2]) for e in ents], [len(e[2]) for e in ents],
                              method=8, kind=kind, **kw)
    raw = _relabel(z, [e[1] for e in ents], kind)
    with open(path, "wb") as f:
        f.write(raw)
    return raw


def _bytes_of(r, i, n):
    o = int(r["out_off"][i])
    return r["out"].cpu().numpy()[o:o + n].tobytes()


def test_archive_mixing_methods(gpu, tmp_path):
    ents = _mixed()
    path = str(tmp_path / "mixed.zip")
    _write(path, ents)
    a = _archive(path)
    assert [int(m) for m in a.table[:, 0]] == [e[1] for e in ents]
    r = a.decode()
    assert list(r["status"]) == [0] * len(ents) and r["ok"].all()
    for i, (name, _, data, _) in enumerate(ents):
        assert int(r["out_len"][i]) == len(data) and _bytes_of(r, i, len(data)) == data and int(r["crc"][i]) == zlib.crc32(data), name
    r = a.decode(lo=7, hi=11)   # a slice of method-93 entries alone
    assert list(r["status"]) == [0, 0, 0, 0] and _bytes_of(r, 1, len(ents[8][2])) == ents[8][2]


def test_archive_with_damaged_zstd_entries(gpu, tmp_path):
    """a flipped payload byte fails that entry alone, as expand() reads it; a directory CRC that names other bytes is a CRC error"""
    ents = _mixed()
    path = str(tmp_path / "damaged.zip")
    raw = bytearray(_write(path, ents))
    p2 = raw.index(ents[2][3])
    raw[p2 + len(ents[2][3]) // 2] ^= 0x40
    want2 = zf.expand(bytes(raw[p2:p2 + len(ents[2][3])]), len(ents[2][2]))[0]
    assert want2 != 0
    cd = -4
    for _ in range(8):             # the directory record of entry 7: its CRC field names other bytes
        cd = raw.index(b"PK\x01\x02", cd + 4)
    raw[cd + 16:cd + 20] = struct.pack("<I", zlib.crc32(ents[7][2]) ^ 0x00100000)
    with open(path, "wb") as f:
        f.write(raw)
    r = _archive(path).decode()
    want = [0] * len(ents)
    want[2], want[7] = want2, cr.MZ_CRC_ERROR
    assert list(r["status"]) == want and list(r["ok"]) == [w == 0 for w in want]
    for i, (name, _, data, _) in enumerate(ents):
        if want[i] == 0:
            assert _bytes_of(r, i, len(data)) == data, name


@pytest.mark.parametrize("kind,ae_version", [("pk", 2), ("aes", 1), ("aes", 2)])
def test_encrypted_archives_with_zstd_entries(gpu, tmp_path, kind, ae_version):
    picks = ("text_3k_l19", "one_byte_l3", "empty_l3", "noise_3k_l3", "text_64k_l-5")
    ents = []
    for i, (name, z, d) in enumerate(p for p in zf.payloads() if p[0] in picks):
        crc = zlib.crc32(d)
        if kind == "pk":   # no data descriptor: the check bytes are the CRC's two high bytes
            pay = cr.pk_encrypt(PW, z, (crc >> 16) & 255, crc >> 24, header_seed=i + 1)
        else:              # (assemble_archive writes one strength per archive)
            pay = cr.wz_encrypt(PW, z, 2, salt_seed=i + 1)
        ents.append((name, 93, d, pay))
    assert len(ents) == len(picks)
    path = str(tmp_path / "enc.zip")
    _write(path, ents, kind=kind, strength=2, ae_version=ae_version)
    a = _archive(path)
    r = a.decode(password=PW)
    assert list(r["status"]) == [0] * len(ents) and r["ok"].all()
    for i, (name, _, d, _) in enumerate(ents):
        assert int(r["out_len"][i]) == len(d) and _bytes_of(r, i, len(d)) == d, name
    assert (a.decode()["status"] == cr.MZ_SUPPORT_ERROR).all()
    assert (a.decode(password=b"test124")["status"] != 0).all()


def test_reference_seed_archive_as_method_93(gpu, tmp_path):
    """the reference's fuzzer seed license_zstd.zip holds one real zstd frame under the obsolete method number 20"""
    raw = bytearray(open(os.path.join(ROOT, "tests", "golden", "license_zstd.zip"), "rb").read())
    cd = raw.index(b"PK\x01\x02")
    assert raw[8:10] == b"\x14\x00" and raw[cd + 10:cd + 12] == b"\x14\x00"
    raw[8:10] = raw[cd + 10:cd + 12] = b"\x5d\x00"
    path = str(tmp_path / "license.zip")
    with open(path, "wb") as f:
        f.write(raw)
    a = _archive(path)
    r = a.decode()
    assert list(r["status"]) == [0] and int(r["out_len"][0]) == 894 and r["ok"].all()
    assert int(r["crc"][0]) == int.from_bytes(raw[cd + 16:cd + 20], "little")
