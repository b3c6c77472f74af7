"""CPU tests that pin tests/crypt_ref.py, the judge of the crypt tests: published AES vectors, the reference project's two
seed archives under tests/golden/, and the standard zipfile module reading what the writer wrote."""
import io
import os
import struct
import zipfile

import numpy as np
import pytest

from tests import crypt_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = b"Hello, World!\n"


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
        return f.read()


def first_entry(z):
    """(flag, method, crc, time, date, payload bytes, extra) of the first local header, sizes from the central directory"""
    cd = z.index(b"PK\x01\x02")
    flag, method, tm, dt, crc, csize = struct.unpack_from("<HHHHII", z, cd + 8)
    fn, ex = struct.unpack_from("<HH", z, cd + 28)
    extra = z[cd + 46 + fn:cd + 46 + fn + ex]
    while len(extra) >= 4 and struct.unpack_from("<H", extra)[0] != 0x9901:   # step to the AES field, if there is one
        extra = extra[4 + struct.unpack_from("<H", extra, 2)[0]:]
    lfn, lex = struct.unpack_from("<HH", z, 26)
    p = 30 + lfn + lex
    return flag, method, crc, tm, dt, z[p:p + csize], extra


@pytest.mark.parametrize("key,want", [
    ("000102030405060708090a0b0c0d0e0f", "69c4e0d86a7b0430d8cdb78070b4c55a"),
    ("000102030405060708090a0b0c0d0e0f1011121314151617", "dda97ca4864cdfe06eaf70a0ec0d7191"),
    ("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", "8ea2b7ca516745bfeafc49904b496089")])
def test_fips197_appendix_c(key, want):
    pt = np.frombuffer(bytes.fromhex("00112233445566778899aabbccddeeff"), dtype=np.uint8).reshape(1, 16)
    assert cr.aes_encrypt_blocks(bytes.fromhex(key), pt).tobytes().hex() == want


def test_seed_archive_pkcrypt():
    flag, method, crc, tm, dt, pay, _ = first_entry(golden("encrypted_pkcrypt.zip"))
    assert flag == 9 and method == 0 and len(pay) == 12 + len(TEXT)
    c10, c11 = cr.pk_check_bytes(crc, tm, dt, flag)
    assert cr.pk_decrypt(b"test123", pay, c11 | c10 << 8) == (0, TEXT)
    # (byte 10 of this Info-ZIP-style header is the time's LOW byte; mz_zip_get_pk_verify expects the date's low byte there,
    # and the reference never compares it for a version-needed of 2.0 and above -- nor does the word above ask for it)
    assert cr.pk_decrypt(b"test123", pay, c11 | c10 << 8 | 0x10000)[0] == cr.MZ_PASSWORD_ERROR
    assert cr.pk_decrypt(b"test124", pay, c11 | c10 << 8)[0] == cr.MZ_PASSWORD_ERROR


def test_seed_archive_wzaes():
    flag, method, crc, tm, dt, pay, extra = first_entry(golden("encrypted_wzaes.zip"))
    fid, fsz, ver, vendor, strength, real = struct.unpack("<HHH2sBH", extra[:11])
    assert (flag & 1, method, crc, fid, fsz, ver, vendor, strength, real) == (1, 99, 0, 0x9901, 7, 2, b"AE", 3, 0)
    assert len(pay) == 16 + 2 + len(TEXT) + 10
    assert cr.wz_decrypt(b"test123", pay, 3) == (0, TEXT)
    assert cr.wz_decrypt(b"test124", pay, 3)[0] == cr.MZ_PASSWORD_ERROR
    bad = bytearray(pay)
    bad[20] ^= 1
    assert cr.wz_decrypt(b"test123", bytes(bad), 3)[0] == cr.MZ_CRC_ERROR


@pytest.mark.parametrize("dd", [False, True])
@pytest.mark.parametrize("method", [0, 8])
def test_zipfile_reads_what_the_writer_wrote(dd, method):
    rnd = np.random.RandomState(3)
    ents = [("a.txt", b"alpha " * 50), ("empty", b""), ("r.bin", rnd.bytes(3000))]
    z = cr.write_zip(ents, password=b"s3cret", kind="pk", method=method, data_descriptor=dd)
    with zipfile.ZipFile(io.BytesIO(z)) as f:
        for name, data in ents:
            assert f.getinfo(name).flag_bits & 9 == (9 if dd else 1)
            assert f.read(name, pwd=b"s3cret") == data
        with pytest.raises(RuntimeError):
            f.read("a.txt", pwd=b"s3cres")


def test_zipfile_reads_plain_entries_of_a_mixed_archive():
    ents = [dict(name="p", data=b"plain" * 9), dict(name="d", data=b"deflate " * 99, method=8),
            dict(name="k", data=b"secret", kind="pk", password=b"pw"),
            dict(name="x", data=b"aes " * 40, kind="aes", password=b"pw", strength=1, ae_version=1, method=8)]
    z = cr.write_zip(ents)
    with zipfile.ZipFile(io.BytesIO(z)) as f:
        assert f.read("p") == ents[0]["data"] and f.read("d") == ents[1]["data"]
        assert f.read("k", pwd=b"pw") == b"secret"
        assert f.getinfo("x").compress_type == 99


def test_wz_roundtrip_and_counter_carry():
    """the keystream counter is little endian: blocks 255 / 256 differ in the first two counter bytes"""
    rnd = np.random.RandomState(5)
    for s in (1, 2, 3):
        d = rnd.bytes(4097 + s)
        e = cr.wz_encrypt(b"pw", d, s)
        assert len(e) == len(d) + 4 * s + 16
        assert cr.wz_decrypt(b"pw", e, s) == (0, d)
    key = bytes(range(16))
    ks = cr.aes_ctr_winzip(key, bytes(16 * 257))
    blk = np.zeros((1, 16), np.uint8)
    blk[0, 1] = 1                                    # counter 256 = 00 01 00 .. (little endian)
    assert ks[16 * 255:16 * 256] == cr.aes_encrypt_blocks(key, blk).tobytes()
