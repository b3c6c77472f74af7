"""The independent judge of the crypt tests: ZipCrypto (APPNOTE 6.1) and WinZip AES (AE-1 / AE-2) in Python, written from
the specifications, with no product code.  AES is numpy-vectorised over all blocks at once (FIPS-197 as stated: SubBytes,
ShiftRows, MixColumns, AddRoundKey on an [n, 16] byte array); PBKDF2 and HMAC come from the standard library.  write_zip
emits archives with encrypted entries for the DeviceArchive tests.  tests/test_crypt_ref.py pins all of it to published
vectors, to the two seed archives under tests/golden/ and to the standard zipfile module."""
import functools
import hashlib
import hmac
import lzma
import struct
import zlib

import numpy as np

MZ_OK, MZ_PARAM_ERROR, MZ_FORMAT_ERROR, MZ_CRC_ERROR, MZ_PASSWORD_ERROR, MZ_SUPPORT_ERROR, MZ_READ_ERROR = 0, -102, -103, -105, -108, -109, -115

# ---- ZipCrypto ---------------------------------------------------------------------------------------------------

_CRC_TAB = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TAB.append(_c)


class PkKeys:
    def __init__(self, password):
        self.k0, self.k1, self.k2 = 305419896, 591751049, 878082192
        for c in password:
            self.update(c)

    def update(self, c):
        self.k0 = _CRC_TAB[(self.k0 ^ c) & 255] ^ (self.k0 >> 8)
        self.k1 = ((self.k1 + (self.k0 & 255)) * 134775813 + 1) & 0xFFFFFFFF
        self.k2 = _CRC_TAB[(self.k2 ^ (self.k1 >> 24)) & 255] ^ (self.k2 >> 8)

    def stream_byte(self):
        t = (self.k2 | 2) & 0xFFFF
        return ((t * (t ^ 1)) >> 8) & 255


def pk_encrypt(password, data, check10, check11, header_seed=1):
    """-> 12-byte encryption header + ciphertext.  Header bytes 0..9 are seeded noise, 10 and 11 the check bytes."""
    k = PkKeys(password)
    head = bytes(np.random.RandomState(header_seed).randint(0, 256, size=10, dtype=np.uint8)) + bytes([check10, check11])
    out = bytearray()
    for c in head + bytes(data):
        out.append(c ^ k.stream_byte())
        k.update(c)
    return bytes(out)


def pk_decrypt(password, entry, verify):
    """verify as mzhip_pkcrypt_batch's d_verify word -> (status, plaintext)"""
    if len(entry) < 12:
        return MZ_READ_ERROR, b""
    k = PkKeys(password)
    out = bytearray()
    for i, c in enumerate(entry):
        if i == 12 and (out[11] != (verify & 255) or ((verify & 0x10000) and out[10] != ((verify >> 8) & 255))):
            break
        p = c ^ k.stream_byte()
        k.update(p)
        out.append(p)
    if out[11] != (verify & 255) or ((verify & 0x10000) and out[10] != ((verify >> 8) & 255)):
        return MZ_PASSWORD_ERROR, b""
    return MZ_OK, bytes(out[12:])


def pk_check_bytes(crc, dos_time, dos_date, flag):
    """(byte 10's, byte 11's) check values: mz_zip_get_pk_verify"""
    if flag & 8:
        return dos_date & 255, (dos_time >> 8) & 255
    return (crc >> 16) & 255, (crc >> 24) & 255


# ---- AES (FIPS-197), all blocks at once ------------------------------------------------------------------------------

def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = ((a << 1) ^ 0x11B) if a & 0x80 else a << 1
        b >>= 1
    return r


def _make_sbox():
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    rot = lambda x, n: ((x << n) | (x >> (8 - n))) & 255   # noqa: E731
    return np.array([inv[a] ^ rot(inv[a], 1) ^ rot(inv[a], 2) ^ rot(inv[a], 3) ^ rot(inv[a], 4) ^ 0x63 for a in range(256)],
                    dtype=np.uint8)


SBOX = _make_sbox()
_SHIFT_ROWS = np.array([(4 * ((c + r) % 4) + r) for c in range(4) for r in range(4)])   # state byte 4c + r <- column c + r


def _xtime(a):
    return ((a << 1) ^ np.where(a & 0x80, 0x1B, 0)).astype(np.uint8)


@functools.lru_cache(maxsize=256)
def _expand_key_cached(key):
    nk = len(key) // 4
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = t[1:] + t[:1]
            t = [int(SBOX[b]) for b in t]
            t[0] ^= rcon
            rcon = _gmul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = [int(SBOX[b]) for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return np.array(w, dtype=np.uint8).reshape(nr + 1, 16), nr


def aes_expand_key(key):
    """-> (round keys uint8 [rounds + 1, 16], rounds)"""
    return _expand_key_cached(bytes(key))


def aes_encrypt_blocks(key, blocks):
    """blocks: uint8 [n, 16] -> uint8 [n, 16]"""
    rk, nr = aes_expand_key(key)
    s = blocks ^ rk[0]
    for r in range(1, nr + 1):
        s = SBOX[s][:, _SHIFT_ROWS]
        if r < nr:
            c = s.reshape(-1, 4, 4)
            a0, a1, a2, a3 = c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3]
            x0, x1, x2, x3 = _xtime(a0), _xtime(a1), _xtime(a2), _xtime(a3)
            s = np.stack([x0 ^ x1 ^ a1 ^ a2 ^ a3, a0 ^ x1 ^ x2 ^ a2 ^ a3, a0 ^ a1 ^ x2 ^ x3 ^ a3, x0 ^ a0 ^ a1 ^ a2 ^ x3],
                         axis=2).reshape(-1, 16)
        s = s ^ rk[r]
    return s


@functools.lru_cache(maxsize=1024)
def _keystream_cached(key, nblk):
    ctr = np.zeros((nblk, 16), dtype=np.uint8)
    ctr[:, :8] = np.arange(1, nblk + 1, dtype="<u8").view(np.uint8).reshape(nblk, 8)
    return aes_encrypt_blocks(key, ctr).reshape(-1)


def aes_ctr_winzip(key, data):
    """XOR with the WinZip keystream: block j (from 0) = AES_k(LE64(j + 1) || 0^8)"""
    n = len(data)
    if n == 0:
        return b""
    nblk = (n + 15) // 16
    # (short entries under one key share their first eight keystream blocks: the many-entry tests encrypt thousands)
    ks = _keystream_cached(bytes(key), 8)[:n] if nblk <= 8 else _keystream_cached.__wrapped__(bytes(key), nblk)[:n]
    return (np.frombuffer(bytes(data), dtype=np.uint8) ^ ks).tobytes()


# ---- WinZip AES entries -----------------------------------------------------------------------------------------------

def wz_keys(password, salt, strength):
    """-> (AES key, HMAC key, 2-byte verifier)"""
    return _wz_keys_cached(bytes(password), bytes(salt), strength)


@functools.lru_cache(maxsize=4096)
def _wz_keys_cached(password, salt, strength):
    klen = 8 * strength + 8
    km = hashlib.pbkdf2_hmac("sha1", bytes(password), bytes(salt), 1000, 2 * klen + 2)
    return km[:klen], km[klen:2 * klen], km[2 * klen:]


def wz_encrypt(password, data, strength, salt_seed=1):
    """-> salt | verifier | ciphertext | authcode"""
    salt = bytes(np.random.RandomState(salt_seed).randint(0, 256, size=4 * strength + 4, dtype=np.uint8))
    ek, hk, ver = wz_keys(password, salt, strength)
    ct = aes_ctr_winzip(ek, data)
    return salt + ver + ct + hmac.new(hk, ct, hashlib.sha1).digest()[:10]


def wz_decrypt(password, entry, strength):
    """-> (status, plaintext) as mzhip_wzaes_batch answers: bytes are delivered with MZ_CRC_ERROR, not with the others"""
    if strength not in (1, 2, 3):
        return MZ_PARAM_ERROR, b""
    sl = 4 * strength + 4
    if len(entry) < sl + 12:
        return MZ_READ_ERROR, b""
    ek, hk, ver = wz_keys(password, entry[:sl], strength)
    if ver != entry[sl:sl + 2]:
        return MZ_PASSWORD_ERROR, b""
    ct = entry[sl + 2:len(entry) - 10]
    st = MZ_OK if hmac.new(hk, ct, hashlib.sha1).digest()[:10] == entry[-10:] else MZ_CRC_ERROR
    return st, aes_ctr_winzip(ek, ct)


# ---- a ZIP writer with encrypted entries -------------------------------------------------------------------------------

def _compress(data, method):
    if method == 0:
        return bytes(data)
    if method == 8:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(bytes(data)) + c.flush()
    if method == 14:   # ZIP-LZMA: version, props size, props, stream with end marker (flag bit 1)
        raw = lzma.compress(bytes(data), format=lzma.FORMAT_ALONE, filters=[dict(id=lzma.FILTER_LZMA1, preset=6)])
        return bytes([5, 2, 5, 0]) + raw[:5] + raw[13:]
    raise ValueError(method)


def write_zip(entries, password=None, kind=None, strength=3, ae_version=2, method=0, data_descriptor=False):
    """entries: (name, data) pairs, or dicts with name / data and any of the keyword arguments as a per-entry override
    (kind: None = plain, "pk" = ZipCrypto, "aes" = WinZip AES), plus crc_xor: damage XORed into the directory's CRC field
    (and the local header's) of that entry.  -> archive bytes.  AE-2 entries carry CRC 0 as WinZip writes them."""
    dflt = dict(password=password, kind=kind, strength=strength, ae_version=ae_version, method=method,
                data_descriptor=data_descriptor, crc_xor=0)
    out, cd = bytearray(), bytearray()
    dos_time, dos_date = (13 << 11) | (37 << 5) | 21, ((2024 - 1980) << 9) | (5 << 5) | 17
    for k, ent in enumerate(entries):
        e = dict(dflt)
        if isinstance(ent, dict):
            e.update(ent)
        else:
            e["name"], e["data"] = ent
        name, data = e["name"].encode(), bytes(e["data"])
        crc = zlib.crc32(data)
        flag = (8 if e["data_descriptor"] else 0) | (2 if e["method"] == 14 else 0)
        payload = _compress(data, e["method"])
        zmethod, extra, need = e["method"], b"", 20
        if e["kind"] == "pk":
            flag |= 1
            c10, c11 = pk_check_bytes(crc, dos_time, dos_date, flag)
            payload = pk_encrypt(e["password"], payload, c10, c11, header_seed=k + 1)
        elif e["kind"] == "aes":
            flag |= 1
            payload = wz_encrypt(e["password"], payload, e["strength"], salt_seed=k + 1)
            extra = struct.pack("<HHH2sBH", 0x9901, 7, e["ae_version"], b"AE", e["strength"], e["method"])
            zmethod, need = 99, 51
            if e["ae_version"] == 2:
                crc = 0
        crc ^= e["crc_xor"]
        off = len(out)
        in_header = (0, 0, 0) if flag & 8 else (crc, len(payload), len(data))
        out += struct.pack("<IHHHHHIIIHH", 0x04034B50, need, flag, zmethod, dos_time, dos_date, *in_header, len(name), len(extra))
        out += name + extra + payload
        if flag & 8:
            out += struct.pack("<IIII", 0x08074B50, crc, len(payload), len(data))
        cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, need, need, flag, zmethod, dos_time, dos_date, crc, len(payload),
                          len(data), len(name), len(extra), 0, 0, 0, 0, off)
        cd += name + extra
    cd_off = len(out)
    out += cd
    out += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(entries), len(entries), len(cd), cd_off, 0)
    return bytes(out)
