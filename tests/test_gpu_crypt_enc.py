"""GPU tests of the write side of the crypt batch path: mzhip_pkcrypt_encrypt_batch / mzhip_wzaes_encrypt_batch through the C ABI,
bit-exact against tests/crypt_ref.py (given the header / salt bytes both formats are fully determined; the tests draw them from
the seeds the judge draws them from), every other byte of the output buffer and the whole input untouched, the round trip
through the read-side calls, the two seed archives reproduced, and encode_archive end to end through DeviceArchive.decode."""
import io
import os
import struct
import zipfile

import numpy as np
import pytest

from tests import crypt_ref as cr
from tests import gpu_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PW, OTHER = b"test123", b"test124"
GUARD = 64
SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025] + list(range(4080, 4113, 8))


@pytest.fixture(scope="module")
def gpu():
    import torch

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    return gpu_util


def _data(n, seed=9):
    return np.random.RandomState(seed + n).bytes(n)


def _over(kind, p):
    return 12 if kind == "pk" else 4 * min(max(int(p), 1), 3) + 16


def rnd_bytes(kind, seed, strength=3):
    """the bytes the judge's pk_encrypt / wz_encrypt draw from `seed`: a 10-byte header, or a 16-byte salt record"""
    if kind == "pk":
        return bytes(np.random.RandomState(seed).randint(0, 256, size=10, dtype=np.uint8))
    k = 4 * min(max(int(strength), 1), 3) + 4
    return bytes(np.random.RandomState(seed).randint(0, 256, size=k, dtype=np.uint8)) + bytes([0xEE] * (16 - k))


def run(kind, datas, param, seeds, in_mis=0, out_mis=0, order=None, password=PW):
    """datas: list of plain byte strings; param: per entry the d_verify word (kind "pk") or the strength (kind "aes"); seeds: per
    entry the seed of its header / salt bytes.  Inputs lie packed behind in_mis bytes, each output slot of len + overhead bytes
    lies between GUARD pattern bytes, the first at out_mis past a 16-byte boundary.  order: the permutation in which the
    entries are handed to the call.  -> (status[n], out_len[n], list of output bytes); asserts that the result arrays were
    written for the n entries only, that the input is unchanged and that nothing outside [out_off, out_off + out_len) of any
    entry was written."""
    import torch

    L = gpu_util.mz.lib()
    n = len(datas)
    in_len = np.array([len(e) for e in datas], dtype=np.int64)
    in_off = in_mis + np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.int64)
    blob = gpu_util.guard_pattern(int(in_mis + in_len.sum() + 16), 77)
    for o, e in zip(in_off, datas):
        blob[o:o + len(e)] = np.frombuffer(e, dtype=np.uint8)
    cap = in_len + np.array([_over(kind, p) for p in param])
    out_off = np.zeros(n, dtype=np.int64)
    pos = 16 * ((GUARD + 15) // 16) + out_mis
    for i in range(n):
        out_off[i] = pos
        pos += int(cap[i]) + GUARD
    fill = gpu_util.guard_pattern(pos + 16, 78)
    idx = np.arange(n) if order is None else np.asarray(order)
    width = 10 if kind == "pk" else 16
    rnd = np.frombuffer(b"".join(rnd_bytes(kind, seeds[i], param[i]) for i in idx), dtype=np.uint8).copy()
    assert rnd.size == width * n
    d_in, d_out, d_rnd = torch.from_numpy(blob).cuda(), torch.from_numpy(fill.copy()).cuda(), torch.from_numpy(rnd).cuda()
    d_in_off, d_out_off = torch.from_numpy(in_off[idx]).cuda(), torch.from_numpy(out_off[idx]).cuda()
    d_in_len = torch.from_numpy(in_len[idx].astype(np.int32)).cuda()
    res = gpu_util.guarded_results(n, ["out_len", "status"])
    if kind == "pk":
        d_par = torch.from_numpy(np.array(param, dtype=np.uint32)[idx].view(np.int32)).cuda()
        rc = L.mzhip_pkcrypt_encrypt_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_out.data_ptr(),
                                           d_out_off.data_ptr(), n, password, len(password), d_par.data_ptr(), d_rnd.data_ptr(),
                                           res["out_len"].data_ptr(), res["status"].data_ptr(), None)
    else:
        d_par = torch.from_numpy(np.array(param, dtype=np.uint8)[idx]).cuda()
        rc = L.mzhip_wzaes_encrypt_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_par.data_ptr(), d_rnd.data_ptr(),
                                         d_out.data_ptr(), d_out_off.data_ptr(), n, password, len(password),
                                         res["out_len"].data_ptr(), res["status"].data_ptr(), None)
    assert rc == 0, (rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    for t in res.values():   # elements behind n untouched, every element in front of it written
        a = t.cpu().numpy().view(np.uint32)
        assert (a[n:] == gpu_util.SENTINEL).all() and (a[:n] != gpu_util.SENTINEL).all()
    status, out_len = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    status[idx] = res["status"].cpu().numpy()[:n]
    out_len[idx] = gpu_util.result_words(res["out_len"], n)
    assert (d_in.cpu().numpy() == blob).all(), "the input was changed"
    assert (d_rnd.cpu().numpy() == rnd).all(), "the header / salt bytes were changed"
    h_out = d_out.cpu().numpy()
    assert (out_len <= cap).all()
    outs = []
    for i in range(n):
        o = int(out_off[i])
        outs.append(h_out[o:o + int(out_len[i])].tobytes())
        h_out[o:o + int(out_len[i])] = fill[o:o + int(out_len[i])]
    bad = np.flatnonzero(h_out != fill)
    assert bad.size == 0, "byte %d of the output buffer, outside every entry's [out_off, out_off + out_len), was written" % int(bad[0])
    return status, out_len, outs


def expect(kind, datas, param, seeds, password=PW):
    """the judge: (status[n], list of output bytes)"""
    st, outs = [], []
    for d, p, s in zip(datas, param, seeds):
        if kind == "pk":
            st.append(0)
            outs.append(cr.pk_encrypt(password, d, (int(p) >> 8) & 255, int(p) & 255, header_seed=s))
        elif int(p) not in (1, 2, 3):
            st.append(cr.MZ_PARAM_ERROR)
            outs.append(b"")
        else:
            st.append(0)
            outs.append(cr.wz_encrypt(password, d, int(p), salt_seed=s))
    return np.array(st, dtype=np.int32), outs


def check(kind, datas, param, seeds, **kw):
    status, out_len, outs = run(kind, datas, param, seeds, **kw)
    want_st, want = expect(kind, datas, param, seeds, password=kw.get("password", PW))
    assert (status == want_st).all(), (np.flatnonzero(status != want_st)[:8], status[status != want_st][:8])
    for i in range(len(datas)):
        assert outs[i] == want[i], (i, len(outs[i]), len(want[i]))
    return status, outs


def decrypt_on_device(kind, entries, param):
    """the read-side calls on what the write side made -> (status[n], list of plaintexts)"""
    from tests.test_gpu_crypt import run as run_read

    status, _, outs = run_read(kind, entries, param, in_mis=3, out_mis=5)
    return status, outs


# ---- sizes, strengths, alignments, counter carry ---------------------------------------------------------------------------

def test_wzaes_encrypt_sizes_and_strengths_and_back(gpu):
    datas, par, seeds = [], [], []
    for s in (1, 2, 3):
        for n in SIZES:
            datas.append(_data(n))
            par.append(s)
            seeds.append(n + s)
    st, outs = check("aes", datas, par, seeds, in_mis=1, out_mis=3)
    assert (st == 0).all()
    st, back = decrypt_on_device("aes", outs, par)
    assert (st == 0).all() and back == datas


def test_pkcrypt_encrypt_sizes_and_back(gpu):
    datas = [_data(n) for n in SIZES]
    st, outs = check("pk", datas, [0x5AC3 | 0x10000] * len(datas), [n + 1 for n in SIZES], in_mis=7, out_mis=2)   # (bit 16 is ignored)
    assert (st == 0).all()
    st, back = decrypt_on_device("pk", outs, [0x5AC3 | 0x10000] * len(datas))
    assert (st == 0).all() and back == datas


@pytest.mark.parametrize("mis", range(16))
def test_every_alignment_at_49_bytes(gpu, mis):
    """16 entries of 49 bytes per launch: inputs lie packed, so entry k reads at alignment mis + 49 k = mis + k (mod 16), and the
    output slots lie 49 + overhead + GUARD = 125 / 133 / 137 / 141 bytes apart -- an odd stride, so the 16 entries write at 16
    different alignments: over the 16 values of mis every one of the 256 (input, output) alignment pairs occurs, for both kinds
    and every strength."""
    d = _data(49)
    for s in (1, 2, 3):
        assert (49 + 4 * s + 16 + GUARD) % 2 == 1
        assert (check("aes", [d] * 16, [s] * 16, list(range(16)), in_mis=mis)[0] == 0).all()
    assert (49 + 12 + GUARD) % 2 == 1
    assert (check("pk", [d] * 16, [0x0102] * 16, list(range(16)), in_mis=mis)[0] == 0).all()


def test_wzaes_counter_carries_at_block_65536(gpu):
    d = _data((1 << 20) + 17)
    st, outs = check("aes", [d, d[:70000]], [2, 3], [1, 1], in_mis=5, out_mis=9)
    assert (st == 0).all()
    st, back = decrypt_on_device("aes", outs, [2, 3])
    assert (st == 0).all() and back == [d, d[:70000]]


# ---- many entries ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """5 000 entries of at most 64 bytes: both kinds, all strengths, at most 61 distinct salt seeds (the judge derives each key
    once), every 7th AES entry with a strength outside 1..3.  The judge's answers are computed once and shared."""
    rnd = np.random.RandomState(2025)
    out = {}
    for kind, n in (("pk", 2500), ("aes", 2500)):
        datas = [rnd.bytes(int(rnd.randint(0, 65))) for _ in range(n)]
        if kind == "pk":
            par = [int(rnd.randint(0, 1 << 16)) for _ in range(n)]
            seeds = list(range(n))
        else:
            par = [(0, 4, 255)[(i // 7) % 3] if i % 7 == 0 else 1 + i % 3 for i in range(n)]
            seeds = [i % 61 for i in range(n)]
        out[kind] = (datas, par, seeds) + expect(kind, datas, par, seeds)
    return out


def test_batch_of_5000_statuses_bytes_guards(gpu, big):
    for kind in ("pk", "aes"):
        datas, par, seeds, want_st, want = big[kind]
        bad = np.arange(len(datas)) % 7 == 0
        assert (want_st[~bad] == 0).all() and (kind == "pk" or (want_st[bad] == cr.MZ_PARAM_ERROR).all())
        status, out_len, outs = run(kind, datas, par, seeds)
        assert (status == want_st).all(), np.flatnonzero(status != want_st)[:8]
        assert outs == want   # (a refused entry: out_len 0, and run() found its slot untouched; its neighbours are whole)


def test_batch_of_5000_in_reverse_order(gpu, big):
    for kind in ("pk", "aes"):
        datas, par, seeds, want_st, want = big[kind]
        status, out_len, outs = run(kind, datas, par, seeds, order=np.arange(len(datas))[::-1])
        assert (status == want_st).all() and outs == want


def test_one_wzaes_call_of_10000_reuses_waves(gpu, big):
    """more entries in one call than the CTR kernel's persistent grid has waves"""
    datas, par, seeds, want_st, want = big["aes"]
    status, out_len, outs = run("aes", datas * 4, par * 4, seeds * 4)
    assert (status == np.tile(want_st, 4)).all() and outs == want * 4


# ---- call level ------------------------------------------------------------------------------------------------------------

def test_call_level_errors(gpu):
    import torch

    L = gpu.mz.lib()
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def pk_args(pw, n, count=1):
        return (z.data_ptr(), None, None, z.data_ptr(), None, count, pw, n, None, None, None, None, None)

    def wz_args(pw, n, count=1):
        return (z.data_ptr(), None, None, None, None, z.data_ptr(), None, count, pw, n, None, None, None)

    assert L.mzhip_pkcrypt_encrypt_batch(*pk_args(None, 0)) == cr.MZ_PARAM_ERROR
    assert L.mzhip_wzaes_encrypt_batch(*wz_args(None, 0)) == cr.MZ_PARAM_ERROR
    assert L.mzhip_wzaes_encrypt_batch(*wz_args(b"x" * 129, 129)) == cr.MZ_PARAM_ERROR
    assert L.mzhip_pkcrypt_encrypt_batch(*pk_args(PW, len(PW), 0)) == 0      # n = 0: nothing is touched, as on the read side
    assert L.mzhip_wzaes_encrypt_batch(*wz_args(PW, len(PW), 0)) == 0
    torch.cuda.synchronize()
    assert int(z.cpu().numpy().max()) == 0
    d = _data(100)
    long_pw = bytes(range(1, 129))
    st, _ = check("aes", [d], [3], [1], password=long_pw)
    assert st[0] == 0
    st, outs = check("aes", [d] * 3, [0, 4, 1], [1, 1, 1])
    assert list(st) == [cr.MZ_PARAM_ERROR, cr.MZ_PARAM_ERROR, 0] and outs[:2] == [b"", b""]


# ---- the reference's own bytes ---------------------------------------------------------------------------------------------

def seed_entry(name):
    z = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
    sig, need, flag, method, tm, dt, crc, csize, usize, fn, ex = struct.unpack("<IHHHHHIIIHH", z[:30])
    assert sig == 0x04034B50 and flag & 1
    if flag & 8:
        cd = z.index(b"PK\x01\x02")
        crc, csize, usize = struct.unpack("<III", z[cd + 16:cd + 28])
    return flag, method, crc, tm, dt, z[30 + fn + ex:30 + fn + ex + csize], z[30 + fn:30 + fn + ex]


def _encrypt_one(kind, data, par, rnd, mis):
    """one entry with the given header / salt-record bytes (not a seed) at input / output misalignment mis -> (status, bytes)"""
    import torch

    L = gpu_util.mz.lib()
    over = _over(kind, par)
    blob = gpu_util.guard_pattern(len(data) + 32, 5)
    blob[mis:mis + len(data)] = np.frombuffer(data, dtype=np.uint8)
    fill = gpu_util.guard_pattern(len(data) + over + 2 * GUARD, 6)
    d_in, d_out = torch.from_numpy(blob).cuda(), torch.from_numpy(fill.copy()).cuda()
    d_rnd = torch.from_numpy(np.frombuffer(rnd, dtype=np.uint8).copy()).cuda()
    d_in_off, d_out_off = torch.tensor([mis], dtype=torch.int64).cuda(), torch.tensor([GUARD - mis], dtype=torch.int64).cuda()
    d_in_len = torch.tensor([len(data)], dtype=torch.int32).cuda()
    res = gpu_util.guarded_results(1, ["out_len", "status"])
    if kind == "pk":
        d_par = torch.tensor([par], dtype=torch.int32).cuda()
        rc = L.mzhip_pkcrypt_encrypt_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_out.data_ptr(),
                                           d_out_off.data_ptr(), 1, PW, len(PW), d_par.data_ptr(), d_rnd.data_ptr(),
                                           res["out_len"].data_ptr(), res["status"].data_ptr(), None)
    else:
        d_par = torch.tensor([par], dtype=torch.uint8).cuda()
        rc = L.mzhip_wzaes_encrypt_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_par.data_ptr(), d_rnd.data_ptr(),
                                         d_out.data_ptr(), d_out_off.data_ptr(), 1, PW, len(PW), res["out_len"].data_ptr(),
                                         res["status"].data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    k = int(gpu_util.result_words(res["out_len"], 1)[0])
    h = d_out.cpu().numpy()
    o = GUARD - mis
    got = h[o:o + k].tobytes()
    h[o:o + k] = fill[o:o + k]
    assert (h == fill).all() and (d_in.cpu().numpy() == blob).all()
    return int(res["status"].cpu().numpy()[0]), got


def test_seed_archive_pkcrypt_is_reproduced(gpu):
    flag, method, crc, tm, dt, pay, _ = seed_entry("encrypted_pkcrypt.zip")
    k = cr.PkKeys(PW)
    plain = bytearray()
    for c in pay:   # the judge's key stream, all 12 header bytes kept
        p = c ^ k.stream_byte()
        k.update(p)
        plain.append(p)
    assert plain[11] == cr.pk_check_bytes(crc, tm, dt, flag)[1]
    assert _encrypt_one("pk", bytes(plain[12:]), plain[11] | plain[10] << 8, bytes(plain[:10]), 5) == (0, pay)


def test_seed_archive_wzaes_is_reproduced(gpu):
    flag, method, crc, tm, dt, pay, extra = seed_entry("encrypted_wzaes.zip")
    fid, fsz, ver, vendor, strength, real = struct.unpack("<HHH2sBH", extra[:11])
    assert method == 99 and fid == 0x9901 and vendor == b"AE"
    st, plain = cr.wz_decrypt(PW, pay, strength)
    assert st == 0
    salt = pay[:4 * strength + 4]
    assert _encrypt_one("aes", plain, strength, salt + bytes(16 - len(salt)), 7) == (0, pay)


# ---- encode_archive end to end ----------------------------------------------------------------------------------------------

def _ar():
    from importlib import import_module

    return import_module("minizip-ng_amd.archive")


WORDS = b"alpha beta gamma delta epsilon zeta eta theta iota kappa lambda " * 1100
ENTRIES = [("empty", b""), ("one", b"x"), ("text.txt", WORDS[7:3000]), ("dir/64k", WORDS[100:100 + 65536]), ("noise.bin", _data(5000))]


def _entropy(k):
    return np.random.RandomState(5).bytes(k)


def wrong_password_fails_the_check_byte_of_the_empty_entry():
    """The end-to-end test asks for a non-zero status on EVERY ZipCrypto entry under a wrong password.  ZipCrypto's check is one
    byte, and an empty stored entry has neither a codec nor a CRC other than 0 to catch what passes it: with the header bytes
    _entropy gives entry 0, the judge says, the wrong password is refused at the check byte."""
    k, e = cr.PkKeys(PW), bytearray()
    for c in _entropy(10 * len(ENTRIES))[:10] + b"\0\0":   # CRC 0: both check bytes are 0
        e.append(c ^ k.stream_byte())
        k.update(c)
    return cr.pk_decrypt(PW, bytes(e), 0)[0] == 0 and cr.pk_decrypt(OTHER, bytes(e), 0)[0] == cr.MZ_PASSWORD_ERROR


CASES = [(None, m, 3, 2) for m in (0, 8, 14)] + [("pk", m, 3, 2) for m in (0, 8, 14)] + \
        [("aes", m, s, v) for m in (0, 8, 14) for s in (1, 2, 3) for v in (1, 2)]


@pytest.mark.parametrize("kind,method,strength,ae_version", CASES)
def test_encode_archive_end_to_end(gpu, tmp_path, kind, method, strength, ae_version):
    ar = _ar()
    pw = None if kind is None else PW
    z = ar.encode_archive(ENTRIES, method=method, password=pw, kind=kind, strength=strength, ae_version=ae_version, entropy=_entropy)
    path = str(tmp_path / "written.zip")
    with open(path, "wb") as f:
        f.write(z)
    a = ar.DeviceArchive(path)
    t = a.table
    assert len(t) == len(ENTRIES)
    cf = ar.crypt_fields(a.h_file, t)
    assert (cf["method"] == method).all() and not cf["format_error"].any()
    assert ((t[:, ar.COL_FLAG] & 1) == (0 if kind is None else 1)).all() and ((t[:, ar.COL_FLAG] & 8) == 0).all()
    if kind == "aes":
        assert (t[:, ar.COL_METHOD] == 99).all() and (cf["aes_version"] == ae_version).all() and (cf["aes_strength"] == strength).all()
        assert ((t[:, ar.COL_CRC] == 0).all()) if ae_version == 2 else (t[3, ar.COL_CRC] != 0)
    r = a.decode(password=pw)
    assert list(r["status"]) == [0] * len(ENTRIES) and r["ok"].all()
    h = r["out"].cpu().numpy()
    for i, (_, d) in enumerate(ENTRIES):
        o = int(r["out_off"][i])
        assert int(r["out_len"][i]) == len(d) and h[o:o + len(d)].tobytes() == d, i
    if kind is not None:
        assert wrong_password_fails_the_check_byte_of_the_empty_entry()
        st = a.decode(password=OTHER)["status"]
        assert (st == cr.MZ_PASSWORD_ERROR).all() if kind == "aes" else (st != 0).all()
        assert (a.decode()["status"] == cr.MZ_SUPPORT_ERROR).all()
    if kind != "aes":   # the standard library reads plain and ZipCrypto archives
        with zipfile.ZipFile(io.BytesIO(z)) as f:
            f.setpassword(pw)
            assert f.testzip() is None and [f.read(n) for n, _ in ENTRIES] == [d for _, d in ENTRIES]


def test_encode_archive_refuses_what_needs_zip64(gpu):
    ar = _ar()
    with pytest.raises(gpu.mz.MzHipError):
        ar.encode_archive([("a", b"")] * 65536, method=0)
    with pytest.raises(gpu.mz.MzHipError):
        ar.encode_archive([("a", b"abc")], kind="pk")
    with pytest.raises(gpu.mz.MzHipError):
        ar.encode_archive([("a", b"abc")], password=PW)
