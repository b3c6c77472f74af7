"""GPU tests of the crypt batch path: mzhip_pkcrypt_batch / mzhip_wzaes_batch through the C ABI against tests/crypt_ref.py
(statuses exact per entry, bytes bit-exact, every other byte of the output buffer and the whole input untouched), and
DeviceArchive.decode(password=...) on the two seed archives and on a written archive that mixes every kind."""
import os

import numpy as np
import pytest

from tests import crypt_ref as cr
from tests import gpu_util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PW, OTHER = b"test123", b"test124"
GUARD = 64
TEXT = b"Hello, World!\n"


@pytest.fixture(scope="module")
def gpu():
    import torch

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    return gpu_util


def _data(n, seed=9):
    return np.random.RandomState(seed + n).bytes(n)


def run(kind, entries, param, in_mis=0, out_mis=0, order=None, password=PW):
    """entries: list of input byte strings (each may be cut or damaged); param: per entry the d_verify word (kind "pk") or the
    strength (kind "aes").  Inputs lie packed behind in_mis bytes (so every alignment occurs), each output slot of the
    undamaged plain length lies between GUARD pattern bytes, the first at out_mis past a 16-byte boundary.  order: the
    permutation in which the entries are handed to the call.  -> (status[n], out_len[n], list of output bytes); asserts that
    the input is unchanged and that nothing outside [out_off, out_off + out_len) of any entry was written."""
    import torch

    L = gpu_util.mz.lib()
    n = len(entries)
    over = [12 if kind == "pk" else 4 * min(max(int(p), 1), 3) + 16 for p in param]
    in_len = np.array([len(e) for e in entries], dtype=np.int64)
    in_off = in_mis + np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.int64)
    blob = gpu_util.guard_pattern(int(in_mis + in_len.sum() + 16), 77)
    for o, e in zip(in_off, entries):
        blob[o:o + len(e)] = np.frombuffer(e, dtype=np.uint8)
    cap = np.maximum(in_len - np.array(over), 0)
    out_off = np.zeros(n, dtype=np.int64)
    pos = 16 * ((GUARD + 15) // 16) + out_mis
    for i in range(n):
        out_off[i] = pos
        pos += int(cap[i]) + GUARD
    fill = gpu_util.guard_pattern(pos + 16, 78)
    idx = np.arange(n) if order is None else np.asarray(order)
    d_in, d_out = torch.from_numpy(blob).cuda(), torch.from_numpy(fill.copy()).cuda()
    d_in_off, d_out_off = torch.from_numpy(in_off[idx]).cuda(), torch.from_numpy(out_off[idx]).cuda()
    d_in_len = torch.from_numpy(in_len[idx].astype(np.int32)).cuda()
    res = gpu_util.guarded_results(n, ["out_len", "status"])
    if kind == "pk":
        d_par = torch.from_numpy(np.array(param, dtype=np.uint32)[idx].view(np.int32)).cuda()
        rc = L.mzhip_pkcrypt_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_out.data_ptr(), d_out_off.data_ptr(),
                                   n, password, len(password), d_par.data_ptr(), res["out_len"].data_ptr(), res["status"].data_ptr(), None)
    else:
        d_par = torch.from_numpy(np.array(param, dtype=np.uint8)[idx]).cuda()
        rc = L.mzhip_wzaes_batch(d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_par.data_ptr(), d_out.data_ptr(),
                                 d_out_off.data_ptr(), n, password, len(password), res["out_len"].data_ptr(),
                                 res["status"].data_ptr(), None)
    assert rc == 0, (rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    for t in res.values():   # elements behind n untouched, every element in front of it written
        a = t.cpu().numpy().view(np.uint32)
        assert (a[n:] == gpu_util.SENTINEL).all() and (a[:n] != gpu_util.SENTINEL).all()
    status, out_len = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    status[idx] = res["status"].cpu().numpy()[:n]
    out_len[idx] = gpu_util.result_words(res["out_len"], n)
    assert (d_in.cpu().numpy() == blob).all(), "the input was changed"
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


def expect(kind, entries, param, password=PW):
    f = cr.pk_decrypt if kind == "pk" else cr.wz_decrypt
    ref = [f(password, e, int(p)) for e, p in zip(entries, param)]
    return np.array([r[0] for r in ref], dtype=np.int32), [r[1] for r in ref]


def check(kind, entries, param, **kw):
    status, out_len, outs = run(kind, entries, param, **kw)
    want_st, want = expect(kind, entries, param)
    assert (status == want_st).all(), (np.flatnonzero(status != want_st)[:8], status[status != want_st][:8])
    for i in range(len(entries)):
        assert outs[i] == want[i], (i, len(outs[i]), len(want[i]))
    return status


SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025] + list(range(4080, 4113, 8))


def test_wzaes_sizes_and_strengths(gpu):
    ents, par = [], []
    for s in (1, 2, 3):
        for n in SIZES:
            ents.append(cr.wz_encrypt(PW, _data(n), s, salt_seed=n + s))
            par.append(s)
    st = check("aes", ents, par, in_mis=1, out_mis=3)
    assert (st == 0).all()


def test_wzaes_counter_carries_at_block_65536(gpu):
    d = _data((1 << 20) + 17)
    st = check("aes", [cr.wz_encrypt(PW, d, 2), cr.wz_encrypt(PW, d[:70000], 3)], [2, 3], in_mis=5, out_mis=9)
    assert (st == 0).all()


def test_pkcrypt_sizes(gpu):
    ents = [cr.pk_encrypt(PW, _data(n), 0x5A, 0xC3, header_seed=n + 1) for n in SIZES]
    st = check("pk", ents, [0xC3] * len(ents), in_mis=7, out_mis=2)
    assert (st == 0).all()


@pytest.mark.parametrize("mis", range(16))
def test_every_alignment_at_49_bytes(gpu, mis):
    """16 entries of 49 bytes per launch: inputs lie packed (an odd stride of 61 / 73 / 77 / 81 bytes) and the output slots
    49 + GUARD = 113 bytes apart, so entry k reads at alignment mis + stride * k and writes at 113 k = k (mod 16): over the
    16 values of mis every one of the 256 (input, output) alignment pairs occurs, for both kinds and every strength."""
    d = _data(49)
    assert GUARD % 16 == 0
    for s in (1, 2, 3):
        ents = [cr.wz_encrypt(PW, d, s, salt_seed=k) for k in range(16)]
        assert len(ents[0]) % 2 == 1
        assert (check("aes", ents, [s] * 16, in_mis=mis) == 0).all()
    ents = [cr.pk_encrypt(PW, d, 1, 2, header_seed=k) for k in range(16)]
    assert (check("pk", ents, [2] * 16, in_mis=mis) == 0).all()


def damaged(kind, i, rnd):
    """entry i of the big batch: (bytes, parameter, wanted status or None = ask the judge)"""
    n = int(rnd.randint(0, 65))
    d = rnd.bytes(n)
    how = (i // 7) % 5 if i % 7 == 0 else -1
    if kind == "pk":
        crc = int(rnd.randint(0, 1 << 32))
        c10, c11 = (crc >> 16) & 255, crc >> 24
        e = cr.pk_encrypt(OTHER if how == 0 else PW, d, c10, c11, header_seed=i)
        v = c11 | c10 << 8
        if how == 1:
            v |= 0x10000                      # second check byte required, and right
        elif how == 2:
            v = (v ^ 0x100) | 0x10000         # ... and wrong
        elif how == 3:
            e = e[:11]                        # one byte short of the header
        elif how == 4:
            v ^= 1                            # check byte wrong
        return e, v
    s = 1 + i % 3
    e = bytearray(cr.wz_encrypt(OTHER if how == 0 else PW, d, s, salt_seed=i % 61))   # (61 salts: the judge derives each key once)
    sl = 4 * s + 4
    if how == 1 and n:
        e[sl + 2 + n // 2] ^= 4                # ciphertext bit
    elif how == 2:
        e[len(e) - 1 - i % 10] ^= 0x80         # authentication-code bit
    elif how == 3:
        e[sl + i % 2] ^= 1                     # verifier bit
    elif how == 4:
        e = e[:sl + 11]                        # one byte short of the overhead
    return bytes(e), s


@pytest.fixture(scope="module")
def big():
    """5 000 entries of at most 64 bytes: more waves than any persistent grid of the library holds; both kinds, all strengths,
    every 7th entry damaged"""
    rnd = np.random.RandomState(2024)
    out = {}
    for kind, n in (("pk", 2500), ("aes", 2500)):
        made = [damaged(kind, i, rnd) for i in range(n)]
        ents, par = [m[0] for m in made], [m[1] for m in made]
        out[kind] = (ents, par) + expect(kind, ents, par)
    return out


def test_batch_of_5000_statuses_bytes_guards(gpu, big):
    for kind in ("pk", "aes"):
        ents, par, want_st, want = big[kind]
        seen = set(int(s) for s in want_st)
        assert {0, cr.MZ_PASSWORD_ERROR, cr.MZ_READ_ERROR} <= seen and (kind == "pk" or cr.MZ_CRC_ERROR in seen)
        assert (want_st[np.arange(len(ents)) % 7 != 0] == 0).all()
        status, out_len, outs = run(kind, ents, par)
        assert (status == want_st).all(), np.flatnonzero(status != want_st)[:8]
        assert outs == want


def test_batch_of_5000_in_reverse_order(gpu, big):
    for kind in ("pk", "aes"):
        ents, par, want_st, want = big[kind]
        status, out_len, outs = run(kind, ents, par, order=np.arange(len(ents))[::-1])
        assert (status == want_st).all() and outs == want


def test_one_wzaes_call_of_5000_reuses_waves(gpu, big):
    """(the two halves above are 2 500 entries each: this one call holds more entries than the CTR kernel's grid has waves)"""
    ents, par, want_st, want = big["aes"]
    status, out_len, outs = run("aes", ents + ents, par + par)
    assert (status == np.concatenate((want_st, want_st))).all() and outs == want + want


def test_call_level_errors(gpu):
    import torch

    L = gpu.mz.lib()
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for fn, args in ((L.mzhip_pkcrypt_batch, lambda pw, n: (z.data_ptr(), None, None, z.data_ptr(), None, 1, pw, n, None, None, None, None)),
                     (L.mzhip_wzaes_batch, lambda pw, n: (z.data_ptr(), None, None, None, z.data_ptr(), None, 1, pw, n, None, None, None))):
        assert fn(*args(None, 0)) == cr.MZ_PARAM_ERROR
    assert L.mzhip_wzaes_batch(*args(b"x" * 129, 129)) == cr.MZ_PARAM_ERROR
    d = _data(100)
    long_pw = bytes(range(1, 129))
    st, _, outs = run("aes", [cr.wz_encrypt(long_pw, d, 3)], [3], password=long_pw)
    assert st[0] == 0 and outs[0] == d
    st, _, outs = run("aes", [cr.wz_encrypt(PW, d, 1)] * 3, [0, 4, 1])
    assert list(st) == [cr.MZ_PARAM_ERROR, cr.MZ_PARAM_ERROR, 0] and outs == [b"", b"", d]


# ---- DeviceArchive -------------------------------------------------------------------------------------------------------

def _archive(path):
    from importlib import import_module

    return import_module("minizip-ng_amd.archive").DeviceArchive(path)


@pytest.mark.parametrize("name", ["encrypted_pkcrypt.zip", "encrypted_wzaes.zip"])
def test_seed_archives(gpu, name):
    a = _archive(os.path.join(ROOT, "tests", "golden", name))
    r = a.decode(password=PW)
    assert list(r["status"]) == [0] and bool(r["ok"][0])
    assert r["out"].cpu().numpy()[:len(TEXT)].tobytes() == TEXT
    assert list(a.decode(password=OTHER)["status"]) == [cr.MZ_PASSWORD_ERROR]
    r = a.decode()
    assert list(r["status"]) == [cr.MZ_SUPPORT_ERROR] and not r["ok"][0]


def test_written_archive_of_every_kind(gpu, tmp_path):
    rnd = np.random.RandomState(31)
    words = (b"alpha beta gamma delta epsilon zeta eta theta iota kappa lambda " * 1100)

    def text(n):
        o = int(rnd.randint(0, 500))
        return words[o:o + n]

    ents = [dict(name="plain0", data=text(700)), dict(name="plain8", data=text(4096), method=8),
            dict(name="empty_pk", data=b"", kind="pk"), dict(name="big_deflate_aes", data=text(65536), kind="aes", method=8, strength=3)]
    for dd in (False, True):
        for m in (0, 8, 14):
            ents.append(dict(name="pk_%d_%d" % (dd, m), data=text(int(rnd.randint(1, 4097))), kind="pk", method=m, data_descriptor=dd))
    for ver in (1, 2):
        for s in (1, 2, 3):
            for m in (0, 8, 14):
                ents.append(dict(name="ae%d_s%d_m%d" % (ver, s, m), data=text(int(rnd.randint(1, 4097))), kind="aes", ae_version=ver,
                                 strength=s, method=m))
    ents.append(dict(name="one_byte_aes", data=b"x", kind="aes", strength=1, ae_version=1))
    bad1 = len(ents)
    ents.append(dict(name="ae1_bad_crc", data=text(900), kind="aes", ae_version=1, strength=2, method=8, crc_xor=0x10))
    bad2 = len(ents)
    ents.append(dict(name="ae2_bad_crc", data=text(900), kind="aes", ae_version=2, strength=2, method=8, crc_xor=0x10))
    path = str(tmp_path / "mixed.zip")
    with open(path, "wb") as f:
        f.write(cr.write_zip(ents, password=PW))
    a = _archive(path)
    r = a.decode(password=PW)
    want = np.zeros(len(ents), dtype=np.int32)
    want[bad1] = cr.MZ_CRC_ERROR
    assert list(r["status"]) == list(want)
    assert list(r["ok"]) == list(want == 0)
    h = r["out"].cpu().numpy()
    for i, e in enumerate(ents):
        o = int(r["out_off"][i])
        assert int(r["out_len"][i]) == len(e["data"]) and h[o:o + len(e["data"])].tobytes() == e["data"], e["name"]
    enc = np.array([e.get("kind") is not None for e in ents])
    r = a.decode()
    assert (r["status"][enc] == cr.MZ_SUPPORT_ERROR).all() and (r["status"][~enc] == 0).all()
    r = a.decode(password=OTHER)
    # (a wrong password passes ZipCrypto's one check byte once in 256: then the codec or the CRC refuses the entry)
    assert (r["status"][enc] != 0).all() and (r["status"][~enc] == 0).all()
    aes = np.array([e.get("kind") == "aes" for e in ents])
    assert (r["status"][aes] == cr.MZ_PASSWORD_ERROR).all()


def test_crypt_fields_refuses_a_foreign_aes_field(gpu, tmp_path):
    z = bytearray(cr.write_zip([dict(name="a", data=b"abc" * 30, kind="aes", password=PW), dict(name="b", data=b"xyz", kind="aes", password=PW)]))
    cd = z.index(b"PK\x01\x02")
    q = z.index(b"\x01\x99\x07\x00", cd)
    z[q + 6] = ord("X")                       # vendor "XE" in the first entry's directory record
    path = str(tmp_path / "foreign.zip")
    with open(path, "wb") as f:
        f.write(bytes(z))
    r = _archive(path).decode(password=PW)
    assert list(r["status"]) == [cr.MZ_FORMAT_ERROR, 0]
