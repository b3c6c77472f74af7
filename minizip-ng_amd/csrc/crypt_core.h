/* crypt_core.h -- the two crypt streams the reference puts between the archive and the codec of a password-protected
 * entry (mz_zip.c, the use_crypt branch of the entry-stack build), both directions (the write side is at the end):
 *   - PKWARE traditional encryption ("ZipCrypto", APPNOTE 6.1): three 32-bit keys updated per byte -- a strictly serial
 *     recurrence, so the parallel axis is entries: one LANE per entry, like k_sha_batch;
 *   - WinZip AES (AE-1 / AE-2): PBKDF2-HMAC-SHA1 (RFC 8018 5.2, RFC 2104) key derivation -- serial chains of 2 x 1000
 *     compressions per 20-byte output block, one lane per (entry, block); AES-CTR (FIPS-197 forward cipher) -- every
 *     16-byte block is independent, one WAVE per entry, a lane per block; HMAC-SHA1 over the ciphertext -- serial
 *     again, one lane per entry.
 * Everything is plain C++ and compiles with -DMZHIP_HOST_EMUL (tests/emul/emul_crypt.cpp).
 */
#ifndef MZHIP_CRYPT_CORE_H
#define MZHIP_CRYPT_CORE_H

#include "hash_core.h"

#define MZ_CRYPT_OK 0
#define MZ_CRYPT_PARAM_ERROR (-102)    /* MZ_PARAM_ERROR */
#define MZ_CRYPT_CRC_ERROR (-105)      /* MZ_CRC_ERROR: the AES authentication code differs */
#define MZ_CRYPT_PASSWORD_ERROR (-108) /* MZ_PASSWORD_ERROR */
#define MZ_CRYPT_READ_ERROR (-115)     /* MZ_READ_ERROR: the entry is shorter than the stream's fixed overhead */

#define MZ_PK_HEADER 12u
#define MZ_WZAES_VERIFY 2u
#define MZ_WZAES_AUTH 10u
#define MZ_WZAES_ITER 1000u
#define MZ_WZAES_PW_MAX 128u /* the reference's password buffer */

/* ---- ZipCrypto ------------------------------------------------------------------------------------------------ */

/* keys <- keys after plain byte c; tab = the raw CRC-32 byte table (crc32_core.h, in LDS) */
MZ_DEV void mz_pk_update(uint32_t &k0, uint32_t &k1, uint32_t &k2, uint32_t c, const uint32_t *tab) {
    k0 = tab[(k0 ^ c) & 255u] ^ (k0 >> 8);
    k1 = (k1 + (k0 & 255u)) * 134775813u + 1u;
    k2 = tab[(k2 ^ (k1 >> 24)) & 255u] ^ (k2 >> 8);
}
MZ_DEV uint32_t mz_pk_stream_byte(uint32_t k2) {
    const uint32_t t = k2 | 2u;
    return ((t * (t ^ 1u)) >> 8) & 255u; /* (only bits 0..15 of t reach bits 8..15 of the product) */
}
MZ_DEV uint32_t mz_pk_decode(uint32_t &k0, uint32_t &k1, uint32_t &k2, uint32_t c, const uint32_t *tab) {
    const uint32_t p = (c ^ mz_pk_stream_byte(k2)) & 255u;
    mz_pk_update(k0, k1, k2, p, tab);
    return p;
}

/* the three keys after the password: they depend on nothing else, so the host computes them once per call */
static inline void mz_pk_init_keys_host(const uint8_t *password, uint32_t n, uint32_t keys[3]) {
    uint32_t k0 = 305419896u, k1 = 591751049u, k2 = 878082192u;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t r = (k0 ^ password[i]) & 255u;
        for (int b = 0; b < 8; b++) r = (r >> 1) ^ ((r & 1u) ? MZ_CRC_POLY : 0u);
        k0 = r ^ (k0 >> 8);
        k1 = (k1 + (k0 & 255u)) * 134775813u + 1u;
        r = (k2 ^ (k1 >> 24)) & 255u;
        for (int b = 0; b < 8; b++) r = (r >> 1) ^ ((r & 1u) ? MZ_CRC_POLY : 0u);
        k2 = r ^ (k2 >> 8);
    }
    keys[0] = k0; keys[1] = k1; keys[2] = k2;
}

/* One entry, by ONE lane: in[0 .. in_len) = 12-byte encryption header + payload, out takes in_len - 12 bytes.
 * verify: bits 0-7 the check byte that plain header byte 11 must equal, bits 8-15 the one for byte 10, bit 16: compare
 * byte 10 too (mz_strm_pkcrypt.c does for version-needed below 2).  Nothing is written unless the header checks out.
 * The payload goes 16 bytes at a time from the first 16-byte boundary of the input on, per byte in front and behind. */
MZ_DEV int32_t mz_pkcrypt_entry(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t verify, uint32_t k0, uint32_t k1,
                                uint32_t k2, const uint32_t *tab, uint32_t *out_len) {
    *out_len = 0;
    if (in_len < MZ_PK_HEADER) return MZ_CRYPT_READ_ERROR;
    uint32_t h10 = 0, h11 = 0;
    for (uint32_t i = 0; i < MZ_PK_HEADER; i++) {
        const uint32_t p = mz_pk_decode(k0, k1, k2, in[i], tab);
        if (i == 10) h10 = p;
        if (i == 11) h11 = p;
    }
    if (h11 != (verify & 255u)) return MZ_CRYPT_PASSWORD_ERROR;
    if ((verify & 0x10000u) && h10 != ((verify >> 8) & 255u)) return MZ_CRYPT_PASSWORD_ERROR;
    const uint8_t *p = in + MZ_PK_HEADER;
    const uint32_t n = in_len - MZ_PK_HEADER;
    uint32_t i = 0;
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)p) & 15u;
    if (head > n) head = n;
    for (; i < head; i++) out[i] = (uint8_t)mz_pk_decode(k0, k1, k2, p[i], tab);
    for (; i + 16u <= n; i += 16u) {
        uint32_t q[4];
        __builtin_memcpy(q, p + i, 16);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint32_t r = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) r |= mz_pk_decode(k0, k1, k2, (q[w] >> (8 * b)) & 255u, tab) << (8 * b);
            q[w] = r;
        }
        __builtin_memcpy(out + i, q, 16);
    }
    for (; i < n; i++) out[i] = (uint8_t)mz_pk_decode(k0, k1, k2, p[i], tab);
    *out_len = n;
    return MZ_CRYPT_OK;
}

/* ---- AES-128 / 192 / 256, forward cipher (FIPS-197) -------------------------------------------------------------- */

MZ_CONST_TABLE uint8_t mz_aes_sbox[256] = {
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76,
    0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0,
    0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
    0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75,
    0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84,
    0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
    0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8,
    0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2,
    0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
    0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb,
    0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79,
    0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
    0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a,
    0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e,
    0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
    0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16};

/* The two tables a kernel stages in LDS: te0[x] = (02.S[x], S[x], S[x], 03.S[x]) from the top byte down -- SubBytes,
 * ShiftRows and MixColumns of one state byte in one look-up; the tables for the other three rows are rotations of it --
 * and the S-box alone, one byte per word, for the last round (which has no MixColumns). */
typedef struct mz_aes_tables {
    uint32_t te0[256];
    uint32_t sbox[256];
} mz_aes_tables;
MZ_DEV void mz_aes_table_entry(mz_aes_tables *t, uint32_t x) {
    const uint32_t s = mz_aes_sbox[x], s2 = ((s << 1) ^ ((s & 0x80u) ? 0x11bu : 0u)) & 255u;
    t->te0[x] = (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
    t->sbox[x] = s;
}

#define MZ_AES_MAX_RK 60 /* 4 x (14 + 1) words for AES-256 */

/* key expansion (FIPS-197 5.2): key_len = 16 / 24 / 32, rk[] receives 4 x (rounds + 1) big-endian words; -> rounds */
MZ_DEV uint32_t mz_aes_expand_key(const uint8_t *key, uint32_t key_len, uint32_t rk[MZ_AES_MAX_RK]) {
    const uint32_t nk = key_len / 4u, rounds = nk + 6u, total = 4u * (rounds + 1u);
    for (uint32_t i = 0; i < nk; i++)
        rk[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) | ((uint32_t)key[4 * i + 2] << 8) | key[4 * i + 3];
    uint32_t rcon = 1;
    for (uint32_t i = nk; i < total; i++) {
        uint32_t t = rk[i - 1];
        if (i % nk == 0) {
            t = (t << 8) | (t >> 24);
            t = ((uint32_t)mz_aes_sbox[t >> 24] << 24) | ((uint32_t)mz_aes_sbox[(t >> 16) & 255u] << 16) |
                ((uint32_t)mz_aes_sbox[(t >> 8) & 255u] << 8) | mz_aes_sbox[t & 255u];
            t ^= rcon << 24;
            rcon = ((rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u)) & 255u;
        } else if (nk > 6u && i % nk == 4u) {
            t = ((uint32_t)mz_aes_sbox[t >> 24] << 24) | ((uint32_t)mz_aes_sbox[(t >> 16) & 255u] << 16) |
                ((uint32_t)mz_aes_sbox[(t >> 8) & 255u] << 8) | mz_aes_sbox[t & 255u];
        }
        rk[i] = rk[i - nk] ^ t;
    }
    return rounds;
}

/* s[0..3] = the block as four big-endian words (one per column), encrypted in place */
MZ_DEV void mz_aes_encrypt(uint32_t s[4], const uint32_t *rk, uint32_t rounds, const mz_aes_tables *t) {
    uint32_t s0 = s[0] ^ rk[0], s1 = s[1] ^ rk[1], s2 = s[2] ^ rk[2], s3 = s[3] ^ rk[3];
    const uint32_t *te0 = t->te0, *sb = t->sbox;
    for (uint32_t r = 1; r < rounds; r++) {
        const uint32_t *k = rk + 4u * r;
        const uint32_t t0 = te0[s0 >> 24] ^ MZ_ROR32(te0[(s1 >> 16) & 255u], 8) ^ MZ_ROR32(te0[(s2 >> 8) & 255u], 16) ^ MZ_ROR32(te0[s3 & 255u], 24) ^ k[0];
        const uint32_t t1 = te0[s1 >> 24] ^ MZ_ROR32(te0[(s2 >> 16) & 255u], 8) ^ MZ_ROR32(te0[(s3 >> 8) & 255u], 16) ^ MZ_ROR32(te0[s0 & 255u], 24) ^ k[1];
        const uint32_t t2 = te0[s2 >> 24] ^ MZ_ROR32(te0[(s3 >> 16) & 255u], 8) ^ MZ_ROR32(te0[(s0 >> 8) & 255u], 16) ^ MZ_ROR32(te0[s1 & 255u], 24) ^ k[2];
        const uint32_t t3 = te0[s3 >> 24] ^ MZ_ROR32(te0[(s0 >> 16) & 255u], 8) ^ MZ_ROR32(te0[(s1 >> 8) & 255u], 16) ^ MZ_ROR32(te0[s2 & 255u], 24) ^ k[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    const uint32_t *k = rk + 4u * rounds;
    s[0] = ((sb[s0 >> 24] << 24) | (sb[(s1 >> 16) & 255u] << 16) | (sb[(s2 >> 8) & 255u] << 8) | sb[s3 & 255u]) ^ k[0];
    s[1] = ((sb[s1 >> 24] << 24) | (sb[(s2 >> 16) & 255u] << 16) | (sb[(s3 >> 8) & 255u] << 8) | sb[s0 & 255u]) ^ k[1];
    s[2] = ((sb[s2 >> 24] << 24) | (sb[(s3 >> 16) & 255u] << 16) | (sb[(s0 >> 8) & 255u] << 8) | sb[s1 & 255u]) ^ k[2];
    s[3] = ((sb[s3 >> 24] << 24) | (sb[(s0 >> 16) & 255u] << 16) | (sb[(s1 >> 8) & 255u] << 8) | sb[s2 & 255u]) ^ k[3];
}

/* ---- HMAC-SHA1 (RFC 2104) and PBKDF2-HMAC-SHA1 (RFC 8018 5.2) ---------------------------------------------------- */

/* The states of SHA-1 after the key block XOR ipad and XOR opad: computed once per key, every HMAC under that key then
 * starts from them.  A key longer than the 64-byte block is hashed first. */
typedef struct mz_hmac_sha1_key {
    uint32_t ipad[5], opad[5];
} mz_hmac_sha1_key;

MZ_DEV void mz_hmac_sha1_init(mz_hmac_sha1_key *hk, const uint8_t *key, uint32_t key_len) {
    uint32_t kw[16];
    if (key_len > 64u) {
        uint32_t d[5];
        mz_sha1_run(key, key_len, d);
#pragma unroll
        for (int i = 0; i < 16; i++) kw[i] = i < 5 ? d[i] : 0u;
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            uint32_t w = 0;
            for (uint32_t b = 0; b < 4u; b++) {
                const uint32_t q = 4u * (uint32_t)i + b;
                w |= (q < key_len ? (uint32_t)key[q] : 0u) << (24 - 8 * b);
            }
            kw[i] = w;
        }
    }
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = kw[i] ^ 0x36363636u;
    mz_sha1_iv(hk->ipad);
    mz_sha1_block(hk->ipad, w);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = kw[i] ^ 0x5c5c5c5cu;
    mz_sha1_iv(hk->opad);
    mz_sha1_block(hk->opad, w);
}

/* the outer pass: digest words of opad-block || inner digest (20 bytes behind a 64-byte prefix: one compression) */
MZ_DEV void mz_hmac_sha1_outer(const mz_hmac_sha1_key *hk, const uint32_t inner[5], uint32_t mac[5]) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = i < 5 ? inner[i] : 0u;
    w[5] = 0x80000000u;
    w[15] = (64u + 20u) * 8u;
#pragma unroll
    for (int i = 0; i < 5; i++) mac[i] = hk->opad[i];
    mz_sha1_block(mac, w);
}

/* mac[0..5) = the digest words (big endian) of HMAC-SHA1(key, msg[0 .. n)) */
MZ_DEV void mz_hmac_sha1(const mz_hmac_sha1_key *hk, const uint8_t *msg, uint64_t n, uint32_t mac[5]) {
    uint32_t inner[5];
#pragma unroll
    for (int i = 0; i < 5; i++) inner[i] = hk->ipad[i];
    mz_sha1_resume(msg, n, inner, 64);
    mz_hmac_sha1_outer(hk, inner, mac);
}

/* HMAC of a 20-byte message held as five words -- the link U_j = PRF(P, U_j-1) of the PBKDF2 chain: two compressions */
MZ_DEV void mz_hmac_sha1_words5(const mz_hmac_sha1_key *hk, const uint32_t msg[5], uint32_t mac[5]) {
    uint32_t w[16], inner[5];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = i < 5 ? msg[i] : 0u;
    w[5] = 0x80000000u;
    w[15] = (64u + 20u) * 8u;
#pragma unroll
    for (int i = 0; i < 5; i++) inner[i] = hk->ipad[i];
    mz_sha1_block(inner, w);
    mz_hmac_sha1_outer(hk, inner, mac);
}

#define MZ_PBKDF2_SALT_MAX 56u /* salt || INT(i) must fit the message buffer of the first link */

/* T_block (block counts from 1) of PBKDF2-HMAC-SHA1 under the key hk = the password: t[0..5) as digest words */
MZ_DEV void mz_pbkdf2_sha1_block(const mz_hmac_sha1_key *hk, const uint8_t *salt, uint32_t salt_len, uint32_t iterations,
                                 uint32_t block, uint32_t t[5]) {
    uint8_t m[MZ_PBKDF2_SALT_MAX + 4u];
    if (salt_len > MZ_PBKDF2_SALT_MAX) salt_len = MZ_PBKDF2_SALT_MAX;
    for (uint32_t i = 0; i < salt_len; i++) m[i] = salt[i];
    m[salt_len] = (uint8_t)(block >> 24);
    m[salt_len + 1] = (uint8_t)(block >> 16);
    m[salt_len + 2] = (uint8_t)(block >> 8);
    m[salt_len + 3] = (uint8_t)block;
    uint32_t u[5];
    mz_hmac_sha1(hk, m, salt_len + 4u, u);
#pragma unroll
    for (int i = 0; i < 5; i++) t[i] = u[i];
    MZ_NOUNROLL
    for (uint32_t j = 1; j < iterations; j++) {
        uint32_t v[5];
        mz_hmac_sha1_words5(hk, u, v);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            u[i] = v[i];
            t[i] ^= v[i];
        }
    }
}

/* ---- WinZip AES entries -------------------------------------------------------------------------------------- */
/* entry = salt(4s + 4) | verifier(2) | ciphertext | authcode(10); key length 8s + 8, strength s = 1..3 */

MZ_DEV uint32_t mz_wzaes_salt_len(uint32_t strength) { return 4u * strength + 4u; }
MZ_DEV uint32_t mz_wzaes_key_len(uint32_t strength) { return 8u * strength + 8u; }
/* PBKDF2 output blocks of 20 bytes that 2 x key_len + 2 bytes of key material take: 2, 3 or 4 */
MZ_DEV uint32_t mz_wzaes_km_blocks(uint32_t strength) { return (2u * mz_wzaes_key_len(strength) + 2u + 19u) / 20u; }

/* what the key step leaves per entry for the CTR and the authentication steps (HBM scratch, plain stores) */
typedef struct mz_wzaes_entry_keys {
    uint32_t rk[MZ_AES_MAX_RK];
    mz_hmac_sha1_key mac;
    uint32_t rounds;
    int32_t status; /* MZ_CRYPT_OK: the verifier matched and rk / mac are valid */
    uint8_t km[80]; /* the PBKDF2 blocks as bytes: AES key | HMAC key | verifier */
} mz_wzaes_entry_keys;

/* the entry's verdict before any key material: MZ_CRYPT_OK, PARAM (strength), READ (shorter than the overhead) */
MZ_DEV int32_t mz_wzaes_precheck(uint32_t in_len, uint32_t strength) {
    if (strength < 1u || strength > 3u) return MZ_CRYPT_PARAM_ERROR;
    if (in_len < mz_wzaes_salt_len(strength) + MZ_WZAES_VERIFY + MZ_WZAES_AUTH) return MZ_CRYPT_READ_ERROR;
    return MZ_CRYPT_OK;
}

/* Key step 1, one lane per (entry, block 0..3): block `b` of the key material into ek->km.  pw = the password's HMAC key. */
MZ_DEV void mz_wzaes_km_block(const mz_hmac_sha1_key *pw, const uint8_t *in, uint32_t in_len, uint32_t strength, uint32_t b,
                              mz_wzaes_entry_keys *ek) {
    if (mz_wzaes_precheck(in_len, strength) != MZ_CRYPT_OK || b >= mz_wzaes_km_blocks(strength)) return;
    uint32_t t[5];
    mz_pbkdf2_sha1_block(pw, in, mz_wzaes_salt_len(strength), MZ_WZAES_ITER, b + 1u, t);
#pragma unroll
    for (int i = 0; i < 5; i++) mz_st4(ek->km + 20u * b + 4u * (uint32_t)i, __builtin_bswap32(t[i]));
}

/* Key step 2, one lane per entry, behind step 1 of all its blocks: verifier, round keys, HMAC pad states -> status */
MZ_DEV int32_t mz_wzaes_finish_keys(const uint8_t *in, uint32_t in_len, uint32_t strength, mz_wzaes_entry_keys *ek,
                                    uint32_t *out_len) {
    *out_len = 0;
    int32_t st = mz_wzaes_precheck(in_len, strength);
    if (st == MZ_CRYPT_OK) {
        const uint32_t sl = mz_wzaes_salt_len(strength), kl = mz_wzaes_key_len(strength);
        if (ek->km[2u * kl] != in[sl] || ek->km[2u * kl + 1u] != in[sl + 1u]) {
            st = MZ_CRYPT_PASSWORD_ERROR;
        } else {
            ek->rounds = mz_aes_expand_key(ek->km, kl, ek->rk); /* straight into the scratch: no indexed private array */
            mz_hmac_sha1_key mk;
            mz_hmac_sha1_init(&mk, ek->km + kl, kl);
            ek->mac = mk;
            *out_len = in_len - sl - MZ_WZAES_VERIFY - MZ_WZAES_AUTH;
        }
    }
    ek->status = st;
    return st;
}

/* CTR step, one WAVE per entry: lane l of pass i takes 16-byte block j = 64 i + l, whose keystream is
 * AES_k(LE64(j + 1) || 0^8) -- only the low eight bytes of the counter carry.  A pass covers a contiguous 1 KiB.  ct and
 * out may have any byte alignment; the last block may be partial and goes per byte.  rk is wave-uniform. */
MZ_DEV void mz_wzaes_ctr(const uint8_t *ct, uint32_t n, uint8_t *out, const uint32_t *rk, uint32_t rounds,
                         const mz_aes_tables *tab) {
    MZ_LANE_DECL
    const uint32_t nblk = (n + 15u) / 16u;
    for (uint32_t base = 0; base < nblk; base += 64u) {
        MZ_LANES {
            const uint32_t j = base + (uint32_t)lane;
            if (j < nblk) {
                const uint64_t ctr = (uint64_t)j + 1u;
                uint32_t s[4] = {__builtin_bswap32((uint32_t)ctr), __builtin_bswap32((uint32_t)(ctr >> 32)), 0u, 0u};
                mz_aes_encrypt(s, rk, rounds, tab);
                const uint32_t o = 16u * j;
                if (o + 16u <= n) {
                    uint32_t q[4];
                    __builtin_memcpy(q, ct + o, 16);
#pragma unroll
                    for (int w = 0; w < 4; w++) q[w] ^= __builtin_bswap32(s[w]);
                    __builtin_memcpy(out + o, q, 16);
                } else {
                    for (uint32_t k = o; k < n; k++) {
                        const uint32_t w = (k - o) >> 2, sh = 24u - 8u * ((k - o) & 3u);
                        const uint32_t ks = (w == 0 ? s[0] : w == 1 ? s[1] : w == 2 ? s[2] : s[3]) >> sh;
                        out[k] = (uint8_t)(ct[k] ^ ks);
                    }
                }
            }
        }
    }
}

/* Authentication step, one lane per entry: HMAC-SHA1 over the CIPHERTEXT, first 10 bytes against the entry's last 10 */
MZ_DEV int32_t mz_wzaes_auth(const uint8_t *in, uint32_t in_len, uint32_t strength, const mz_wzaes_entry_keys *ek) {
    const uint32_t sl = mz_wzaes_salt_len(strength);
    const uint32_t n = in_len - sl - MZ_WZAES_VERIFY - MZ_WZAES_AUTH;
    mz_hmac_sha1_key mk = ek->mac;
    uint32_t mac[5];
    mz_hmac_sha1(&mk, in + sl + MZ_WZAES_VERIFY, n, mac);
    const uint8_t *a = in + in_len - MZ_WZAES_AUTH;
    uint32_t diff = 0;
    for (uint32_t i = 0; i < MZ_WZAES_AUTH; i++) {
        const uint32_t w = i >> 2;
        const uint32_t m = ((w == 0 ? mac[0] : w == 1 ? mac[1] : mac[2]) >> (24u - 8u * (i & 3u))) & 255u;
        diff |= m ^ a[i];
    }
    return diff ? MZ_CRYPT_CRC_ERROR : MZ_CRYPT_OK;
}

/* ---- the write side -------------------------------------------------------------------------------------------- */
/* Both formats are fully determined by the plaintext, the password and the random bytes the CALLER supplies (the 10 free
 * bytes of the ZipCrypto header, the AES salt): there is no entropy source down here. */

MZ_DEV uint32_t mz_pk_encode(uint32_t &k0, uint32_t &k1, uint32_t &k2, uint32_t p, const uint32_t *tab) {
    const uint32_t c = (p ^ mz_pk_stream_byte(k2)) & 255u;
    mz_pk_update(k0, k1, k2, p, tab); /* the keys follow the PLAIN byte in both directions */
    return c;
}

/* One entry, by ONE lane: out[0 .. in_len + 12) = the encrypted 12-byte header + the encrypted payload.  header10 = the ten
 * free header bytes; verify as on the read side: bits 8-15 become plain header byte 10, bits 0-7 byte 11 (bit 16 means
 * nothing here).  The payload goes 16 bytes at a time from the first 16-byte boundary of the INPUT on, as mz_pkcrypt_entry
 * reads it.  An in_len whose out_len does not fit 32 bits: MZ_CRYPT_PARAM_ERROR, nothing written. */
MZ_DEV int32_t mz_pkcrypt_encrypt_entry(const uint8_t *in, uint32_t in_len, uint8_t *out, const uint8_t *header10, uint32_t verify,
                                        uint32_t k0, uint32_t k1, uint32_t k2, const uint32_t *tab, uint32_t *out_len) {
    *out_len = 0;
    if (in_len > 0xFFFFFFFFu - MZ_PK_HEADER) return MZ_CRYPT_PARAM_ERROR;
    for (uint32_t i = 0; i < 10u; i++) out[i] = (uint8_t)mz_pk_encode(k0, k1, k2, header10[i], tab);
    out[10] = (uint8_t)mz_pk_encode(k0, k1, k2, (verify >> 8) & 255u, tab);
    out[11] = (uint8_t)mz_pk_encode(k0, k1, k2, verify & 255u, tab);
    uint8_t *o = out + MZ_PK_HEADER;
    const uint32_t n = in_len;
    uint32_t i = 0;
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)in) & 15u;
    if (head > n) head = n;
    for (; i < head; i++) o[i] = (uint8_t)mz_pk_encode(k0, k1, k2, in[i], tab);
    for (; i + 16u <= n; i += 16u) {
        uint32_t q[4];
        __builtin_memcpy(q, in + i, 16);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint32_t r = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) r |= mz_pk_encode(k0, k1, k2, (q[w] >> (8 * b)) & 255u, tab) << (8 * b);
            q[w] = r;
        }
        __builtin_memcpy(o + i, q, 16);
    }
    for (; i < n; i++) o[i] = (uint8_t)mz_pk_encode(k0, k1, k2, in[i], tab);
    *out_len = n + MZ_PK_HEADER;
    return MZ_CRYPT_OK;
}

/* WinZip AES: out = salt(4s + 4) | verifier(2) | ciphertext(in_len) | authcode(10).  The entry's verdict before any key
 * material: MZ_CRYPT_OK, or PARAM for a strength outside 1..3 and for an in_len whose out_len does not fit 32 bits. */
MZ_DEV int32_t mz_wzaes_enc_precheck(uint32_t in_len, uint32_t strength) {
    if (strength < 1u || strength > 3u) return MZ_CRYPT_PARAM_ERROR;
    if (in_len > 0xFFFFFFFFu - (mz_wzaes_salt_len(strength) + MZ_WZAES_VERIFY + MZ_WZAES_AUTH)) return MZ_CRYPT_PARAM_ERROR;
    return MZ_CRYPT_OK;
}

/* Key step 1, one lane per (entry, block 0..3), as mz_wzaes_km_block with the salt from the caller's record */
MZ_DEV void mz_wzaes_enc_km_block(const mz_hmac_sha1_key *pw, const uint8_t *salt, uint32_t in_len, uint32_t strength, uint32_t b,
                                  mz_wzaes_entry_keys *ek) {
    if (mz_wzaes_enc_precheck(in_len, strength) != MZ_CRYPT_OK || b >= mz_wzaes_km_blocks(strength)) return;
    uint32_t t[5];
    mz_pbkdf2_sha1_block(pw, salt, mz_wzaes_salt_len(strength), MZ_WZAES_ITER, b + 1u, t);
#pragma unroll
    for (int i = 0; i < 5; i++) mz_st4(ek->km + 20u * b + 4u * (uint32_t)i, __builtin_bswap32(t[i]));
}

/* Key step 2, one lane per entry, behind step 1 of all its blocks: nothing to compare -- the lane WRITES salt and verifier
 * to the front of the output and leaves round keys, HMAC pad states and the status in the record -> status */
MZ_DEV int32_t mz_wzaes_enc_finish_keys(const uint8_t *salt, uint32_t in_len, uint32_t strength, uint8_t *out,
                                        mz_wzaes_entry_keys *ek, uint32_t *out_len) {
    *out_len = 0;
    const int32_t st = mz_wzaes_enc_precheck(in_len, strength);
    if (st == MZ_CRYPT_OK) {
        const uint32_t sl = mz_wzaes_salt_len(strength), kl = mz_wzaes_key_len(strength);
        for (uint32_t i = 0; i < sl; i++) out[i] = salt[i];
        out[sl] = ek->km[2u * kl];
        out[sl + 1u] = ek->km[2u * kl + 1u];
        ek->rounds = mz_aes_expand_key(ek->km, kl, ek->rk); /* straight into the scratch: no indexed private array */
        mz_hmac_sha1_key mk;
        mz_hmac_sha1_init(&mk, ek->km + kl, kl);
        ek->mac = mk;
        *out_len = in_len + sl + MZ_WZAES_VERIFY + MZ_WZAES_AUTH;
    }
    ek->status = st;
    return st;
}

/* (the CTR step is mz_wzaes_ctr itself, plaintext in, out + salt_len + 2: CTR is its own inverse) */

/* Authentication step, one lane per entry, BEHIND the CTR step: HMAC-SHA1 over the ciphertext that step wrote into out,
 * first 10 bytes stored behind it */
MZ_DEV void mz_wzaes_enc_auth(uint8_t *out, uint32_t in_len, uint32_t strength, const mz_wzaes_entry_keys *ek) {
    const uint32_t sl = mz_wzaes_salt_len(strength);
    uint8_t *ct = out + sl + MZ_WZAES_VERIFY;
    mz_hmac_sha1_key mk = ek->mac;
    uint32_t mac[5];
    mz_hmac_sha1(&mk, ct, in_len, mac);
    uint8_t *a = ct + in_len;
    for (uint32_t i = 0; i < MZ_WZAES_AUTH; i++) {
        const uint32_t w = i >> 2;
        a[i] = (uint8_t)((w == 0 ? mac[0] : w == 1 ? mac[1] : mac[2]) >> (24u - 8u * (i & 3u)));
    }
}

#endif
