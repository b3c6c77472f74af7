"""CPU tests of minizip-ng_amd/csrc/crypt_core.h through its host build (tests/emul/emul_crypt.cpp, g++ -DMZHIP_HOST_EMUL):
the primitives against published vectors and hashlib, the two entry paths against tests/crypt_ref.py inside patterned
buffers with red zones.  The product path is the HIP build of the same header (tests/test_gpu_crypt.py)."""
import ctypes as C
import hashlib
import hmac
import os
import subprocess

import numpy as np
import pytest

from tests import crypt_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = C.POINTER(C.c_uint8)
RED = 256
PW = b"test123"


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libemul_crypt.so")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"),
                    "-shared", "-fPIC", os.path.join(ROOT, "tests", "emul", "emul_crypt.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.emul_aes_encrypt.restype = None
    L.emul_aes_encrypt.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p]
    L.emul_hmac_sha1.restype = None
    L.emul_hmac_sha1.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint64, C.c_char_p]
    L.emul_pbkdf2_sha1.restype = None
    L.emul_pbkdf2_sha1.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    L.emul_sha1_resume.restype = None
    L.emul_sha1_resume.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint64, C.c_char_p]
    L.emul_pkcrypt.restype = C.c_int32
    L.emul_pkcrypt.argtypes = [_u8p, C.c_uint32, _u8p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.emul_wzaes.restype = C.c_int32
    L.emul_wzaes.argtypes = [_u8p, C.c_uint32, C.c_uint32, _u8p, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def _pattern(n, seed):
    return np.random.RandomState(seed).randint(1, 256, size=n, dtype=np.uint8)


class _Guarded:
    """One entry inside patterned buffers with red zones, at the byte misalignments mis / omis (relative to 16): the core is
    handed exactly in_len bytes and an output slot of cap bytes; check() asserts that the input is unchanged, that no byte
    outside [out, out + out_len) was written (the crypt paths promise out_len, not just the slot), and returns the bytes."""

    def __init__(self, z, cap, mis=0, omis=0):
        self.n, self.cap = len(z), cap
        self.a = _pattern(RED + 16 + len(z) + RED, 201)
        self.i0 = RED + (-(self.a.ctypes.data + RED) % 16) + mis
        self.a[self.i0:self.i0 + len(z)] = np.frombuffer(z, dtype=np.uint8)
        self.a0 = self.a.copy()
        self.out = _pattern(RED + 16 + cap + RED, 202)
        self.o0 = RED + (-(self.out.ctypes.data + RED) % 16) + omis
        self.out0 = self.out.copy()
        self.pin = C.cast(self.a.ctypes.data + self.i0, _u8p)
        self.pout = C.cast(self.out.ctypes.data + self.o0, _u8p)

    def check(self, out_len):
        assert out_len <= self.cap
        assert (self.a == self.a0).all(), "input changed"
        keep = np.ones(self.out.size, dtype=bool)
        keep[self.o0:self.o0 + out_len] = False
        bad = np.flatnonzero((self.out != self.out0) & keep)
        assert bad.size == 0, "byte at offset %d of the output (out_len %d) was written" % (int(bad[0]) - self.o0, out_len)
        return self.out[self.o0:self.o0 + out_len].tobytes()


def run_pk(emu, entry, verify, pw=PW, mis=0, omis=0):
    g = _Guarded(entry, max(len(entry) - 12, 0), mis, omis)
    ol = C.c_uint32(0xFFFFFFFF)
    st = emu.emul_pkcrypt(g.pin, len(entry), g.pout, verify, pw, len(pw), C.byref(ol))
    return st, g.check(ol.value)


def run_wz(emu, entry, strength, pw=PW, mis=0, omis=0):
    g = _Guarded(entry, max(len(entry) - 4 * strength - 16, 0), mis, omis)
    ol = C.c_uint32(0xFFFFFFFF)
    st = emu.emul_wzaes(g.pin, len(entry), strength, g.pout, pw, len(pw), C.byref(ol))
    return st, g.check(ol.value)


SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025] + list(range(4080, 4113, 8))


def _data(n, seed=9):
    return np.random.RandomState(seed + n).bytes(n)


# ---- primitives ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,want", [
    ("000102030405060708090a0b0c0d0e0f", "69c4e0d86a7b0430d8cdb78070b4c55a"),
    ("000102030405060708090a0b0c0d0e0f1011121314151617", "dda97ca4864cdfe06eaf70a0ec0d7191"),
    ("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f", "8ea2b7ca516745bfeafc49904b496089")])
def test_fips197_appendix_c(emu, key, want):
    out = C.create_string_buffer(16)
    k = bytes.fromhex(key)
    emu.emul_aes_encrypt(k, len(k), bytes.fromhex("00112233445566778899aabbccddeeff"), out)
    assert out.raw.hex() == want


RFC2202 = [
    (b"\x0b" * 20, b"Hi There", "b617318655057264e28bc0b6fb378c8ef146be00"),
    (b"Jefe", b"what do ya want for nothing?", "effcdf6ae5eb2fa2d27416d5f184df9c259a7c79"),
    (b"\xaa" * 20, b"\xdd" * 50, "125d7342b9ac11cd91a39af48aa17b4f63f175d3"),
    (bytes(range(1, 26)), b"\xcd" * 50, "4c9007f4026250c6bc8414f9bf50c86c2d7235da"),
    (b"\x0c" * 20, b"Test With Truncation", "4c1a03424b55e07fe7f27be1d58bb9324a9a5a04"),
    (b"\xaa" * 80, b"Test Using Larger Than Block-Size Key - Hash Key First", "aa4ae5e15272d00e95705637ce8a3b55ed402112"),
    (b"\xaa" * 80, b"Test Using Larger Than Block-Size Key and Larger Than One Block-Size Data",
     "e8e99d0f45237d786d6bbaa7965c7808bbff1a91")]


@pytest.mark.parametrize("case", range(7))
def test_rfc2202_hmac_sha1(emu, case):
    key, msg, want = RFC2202[case]
    out = C.create_string_buffer(20)
    emu.emul_hmac_sha1(key, len(key), msg, len(msg), out)
    assert out.raw.hex() == want == hmac.new(key, msg, hashlib.sha1).hexdigest()


@pytest.mark.parametrize("pw,salt,it,n,want", [
    (b"password", b"salt", 1, 20, "0c60c80f961f0e71f3a9b524af6012062fe037a6"),
    (b"password", b"salt", 2, 20, "ea6c014dc72d6f8ccd1ed92ace1d41f0d8de8957"),
    (b"password", b"salt", 4096, 20, "4b007901b765489abead49d926f721d065a429c1"),
    (b"passwordPASSWORDpassword", b"saltSALTsaltSALTsaltSALTsaltSALTsalt", 4096, 25, "3d2eec4fe41c849b80c8d83662c0e44a8b291a964cf2f07038"),
    (b"pass\0word", b"sa\0lt", 4096, 16, "56fa6aa75548099dcc37d7f03425e0c3")])
def test_rfc6070_pbkdf2(emu, pw, salt, it, n, want):
    out = C.create_string_buffer(n)
    emu.emul_pbkdf2_sha1(pw, len(pw), salt, len(salt), it, out, n)
    assert out.raw.hex() == want == hashlib.pbkdf2_hmac("sha1", pw, salt, it, n).hex()


def test_long_password_is_hashed_first(emu):
    """the reference allows passwords up to 128 bytes: beyond 64 the HMAC key is SHA-1(password)"""
    for n in (64, 65, 128):
        pw = bytes(range(1, n + 1))
        out = C.create_string_buffer(66)
        emu.emul_pbkdf2_sha1(pw, n, b"0123456789abcdef", 16, 1000, out, 66)
        assert out.raw == hashlib.pbkdf2_hmac("sha1", pw, b"0123456789abcdef", 1000, 66)


@pytest.mark.parametrize("n", [0, 55, 56, 63, 64, 65, 119])
def test_resumed_sha1(emu, n):
    prefix, msg = _data(64, 1), _data(n, 2)
    out = C.create_string_buffer(20)
    emu.emul_sha1_resume(prefix, 64, msg, n, out)
    assert out.raw == hashlib.sha1(prefix + msg).digest()


# ---- entries -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strength", [1, 2, 3])
def test_wzaes_sizes(emu, strength):
    for n in SIZES:
        d = _data(n)
        e = cr.wz_encrypt(PW, d, strength, salt_seed=n + 1)
        assert cr.wz_decrypt(PW, e, strength) == (0, d)
        assert run_wz(emu, e, strength) == (0, d), n


def test_wzaes_counter_carries_at_block_65536(emu):
    n = (1 << 20) + 17
    d = _data(n)
    e = cr.wz_encrypt(PW, d, 2)
    st, got = run_wz(emu, e, 2, mis=3, omis=5)
    assert st == 0 and got == d


def test_pkcrypt_sizes(emu):
    for n in SIZES:
        d = _data(n)
        e = cr.pk_encrypt(PW, d, 0x5A, 0xC3, header_seed=n + 1)
        assert run_pk(emu, e, 0xC3) == (0, d) == cr.pk_decrypt(PW, e, 0xC3), n


@pytest.mark.parametrize("mis", range(16))
def test_every_alignment_at_49_bytes(emu, mis):
    d = _data(49)
    for omis in range(16):
        for s in (1, 2, 3):
            assert run_wz(emu, cr.wz_encrypt(PW, d, s), s, mis=mis, omis=omis) == (0, d)
        assert run_pk(emu, cr.pk_encrypt(PW, d, 1, 2), 2, mis=mis, omis=omis) == (0, d)


@pytest.mark.parametrize("strength", [1, 2, 3])
def test_wzaes_errors(emu, strength):
    d = _data(333)
    e = cr.wz_encrypt(PW, d, strength)
    sl = 4 * strength + 4
    assert run_wz(emu, e, strength, pw=b"test124") == (cr.MZ_PASSWORD_ERROR, b"") == cr.wz_decrypt(b"test124", e, strength)
    for pos, want in ((sl + 2 + 100, cr.MZ_CRC_ERROR), (len(e) - 3, cr.MZ_CRC_ERROR), (sl + 1, cr.MZ_PASSWORD_ERROR)):
        bad = bytearray(e)
        bad[pos] ^= 0x10
        ref = cr.wz_decrypt(PW, bytes(bad), strength)
        assert ref[0] == want
        assert run_wz(emu, bytes(bad), strength) == ref, pos     # MZ_CRC_ERROR still delivers the decrypted bytes
    assert run_wz(emu, e[:sl + 11], strength) == (cr.MZ_READ_ERROR, b"") == cr.wz_decrypt(PW, e[:sl + 11], strength)
    assert run_wz(emu, cr.wz_encrypt(PW, b"", strength), strength) == (0, b"")
    long_pw = bytes(range(1, 129))
    assert run_wz(emu, cr.wz_encrypt(long_pw, d, strength), strength, pw=long_pw) == (0, d)


def test_wzaes_strength_outside_1_to_3(emu):
    e = cr.wz_encrypt(PW, b"x" * 40, 1)
    g = _Guarded(e, 40)
    ol = C.c_uint32(7)
    for s in (0, 4, 255):
        assert emu.emul_wzaes(g.pin, len(e), s, g.pout, PW, len(PW), C.byref(ol)) == cr.MZ_PARAM_ERROR
        assert g.check(ol.value) == b""


def test_pkcrypt_errors_and_second_check_byte(emu):
    d = _data(100)
    e = cr.pk_encrypt(PW, d, 0x11, 0x22)
    assert run_pk(emu, e, 0x22, pw=b"test124")[0] == cr.pk_decrypt(b"test124", e, 0x22)[0] == cr.MZ_PASSWORD_ERROR
    assert run_pk(emu, e, 0x23) == (cr.MZ_PASSWORD_ERROR, b"")
    assert run_pk(emu, e, 0x22 | 0x9900) == (0, d)                               # byte 10 differs but is not asked for
    assert run_pk(emu, e, 0x22 | 0x1100 | 0x10000) == (0, d) == cr.pk_decrypt(PW, e, 0x22 | 0x1100 | 0x10000)
    assert run_pk(emu, e, 0x22 | 0x9900 | 0x10000) == (cr.MZ_PASSWORD_ERROR, b"") == cr.pk_decrypt(PW, e, 0x22 | 0x9900 | 0x10000)
    assert run_pk(emu, e[:11], 0x22) == (cr.MZ_READ_ERROR, b"") == cr.pk_decrypt(PW, e[:11], 0x22)
    assert run_pk(emu, e[:12], 0x22) == (0, b"")


def test_sanitised_standalone_program():
    """the same entry points from a program of their own under -fsanitize=address,undefined (exact-size heap buffers)"""
    out = os.path.join(ROOT, "tests", "emul", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "emul_crypt_san")
    subprocess.run(["g++", "-O1", "-g", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DEMUL_CRYPT_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"),
                    os.path.join(ROOT, "tests", "emul", "emul_crypt.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr[-2000:])
