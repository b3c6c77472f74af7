/* bzip2_core.h -- one bzip2 stream (ZIP method 12, the reference's mz_strm_bzip.c over libbz2) decoded by one wave.
 *
 * Written in the wave.h vocabulary: the same text is the gfx950 kernel body (k_bzip2_batch) and, under
 * g++ -DMZHIP_HOST_EMUL, the host build the CPU tests run (tests/emul/emul_bzip2.cpp).  libbz2's decoder is the model
 * for every decision: fields are read in its order and at its granularity (a byte is taken from the input only when a
 * bit of it is needed), so "the input ended" (MZHIP_BUF_ERROR) and "the data is wrong" (MZHIP_DATA_ERROR) fall exactly
 * where BZ2_bzDecompress puts them.  The one deviation: a block with the "randomised" bit set is MZHIP_UNSUPPORTED.
 *
 * Per block a wave
 *   1. parses the header (wave-uniform, bit by bit), builds limit / base / perm per table as BZ2_hbCreateDecodeTables
 *      does -- counts by LDS atomics, perm with a lane per symbol;
 *   2. runs the Huffman / RUNA-RUNB / MTF loop, wave-uniform; the bytes of the block (the BWT's last column) go to the
 *      scratch's byte array, runs are filled and the MTF list is shifted by the lanes;
 *   3. prefix-sums the 256 byte counts (4 per lane + one wave scan);
 *   4. scatters the links, 64 consecutive positions per step: the counting sort is stable, a lane's slot is cftab[byte]
 *      + the number of lower lanes with the same byte (eight ballots over the byte's bits give the same-byte mask).
 *      tt[slot] = position << 8 | byte: the byte of the FIRST column at slot, so the walk needs one load per step;
 *   5. walks the chain from origPtr, serially, undoing the final run-length stage as it goes: bytes go straight to the
 *      output (runs by the lanes), the block CRC (MSB-first, 0x04C11DB7) is folded byte by byte;
 *   6. after the stream's end folds the ZIP CRC-32 over the finished bytes with the K2 tiles.
 *
 * Input is read at BYTE granularity, 256 bytes at a time into LDS, never outside [in, in + in_len).
 * LDS: sizeof(mz_bz_lds) = 9.4 KiB per wave.  Scratch in HBM per wave: MZ_BZ_SCRATCH_BYTES = 4 518 144 (tt: 4 x 900 000,
 * the block's bytes: 900 000, selectors: 18 002).
 */
#ifndef MZHIP_BZIP2_CORE_H
#define MZHIP_BZIP2_CORE_H

#include "crc32_core.h"
#include "wave.h"

#define MZ_BZ_BLOCK_MAX 900000u
#define MZ_BZ_MAX_SELECTORS 18002u
#define MZ_BZ_GROUPS 6u
#define MZ_BZ_ALPHA 258u
#define MZ_BZ_LENS 24u /* limit / base are indexed by code length 0 .. 22 (BZ_MAX_CODE_LEN 23) */
#define MZ_BZ_INBUF 256u
#define MZ_BZ_L_OFF (MZ_BZ_BLOCK_MAX * 4u)
#define MZ_BZ_SEL_OFF (MZ_BZ_L_OFF + MZ_BZ_BLOCK_MAX)
#define MZ_BZ_SCRATCH_BYTES 4518144u /* MZ_BZ_SEL_OFF + 18 002, rounded up to 256 */

typedef struct mz_bz_lds {
    int32_t limit[MZ_BZ_GROUPS][MZ_BZ_LENS];
    int32_t base[MZ_BZ_GROUPS][MZ_BZ_LENS];
    uint16_t perm[MZ_BZ_GROUPS][MZ_BZ_ALPHA];
    uint8_t len[MZ_BZ_GROUPS][260];
    uint32_t unzftab[256];
    uint32_t cftab[256];
    uint32_t bzcrc[256];
    uint8_t mtf[256];
    uint8_t seq2unseq[256];
    uint8_t inbuf[MZ_BZ_INBUF];
    uint8_t minlen[8];
} mz_bz_lds;

typedef struct mz_bz_result {
    uint32_t out_len; /* status 0: the stream's bytes; otherwise the bytes of the blocks in front of the problem that checked out */
    uint32_t in_used; /* status 0: whole bytes through the one holding the last bit of the combined CRC */
    uint32_t crc;     /* CRC-32 of out[0 .. out_len) */
    int32_t status;
} mz_bz_result;

typedef struct mz_bz_bits {
    const uint8_t *in;
    uint32_t in_len;
    uint32_t pos;  /* next byte of the input to take */
    uint32_t base; /* offset of inbuf[0] in the input */
    uint32_t acc, cnt;
} mz_bz_bits;

/* measurement builds (make PROF=1): cycles of the stages, summed over all waves, in mz_prof_buf[28 .. 31]:
 * 28 header + symbol loop, 29 prefix sum + scatter, 30 chain walk + output (one loop), 31 CRC-32 fold */
#if defined(MZ_PROF) && !defined(MZHIP_HOST_EMUL)
#define MZ_BZPROF_DECL uint32_t prof_acc = 0; uint64_t prof_t0 = __builtin_readcyclecounter();
#define MZ_BZPROF_MARK(i)                                                         \
    do {                                                                          \
        const uint32_t _pd = (uint32_t)(__builtin_readcyclecounter() - prof_t0);  \
        prof_acc += (lane == 28 + (i)) ? _pd : 0u;                                \
        prof_t0 = __builtin_readcyclecounter();                                   \
    } while (0)
#define MZ_BZPROF_FLUSH if (lane >= 28 && lane < 32) atomicAdd(&mz_prof_buf[lane], (unsigned long long)prof_acc);
#else
#define MZ_BZPROF_DECL
#define MZ_BZPROF_MARK(i) ((void)0)
#define MZ_BZPROF_FLUSH
#endif

/* the next input byte, or -1 behind the end; the LDS window is refilled by the lanes, 4 bytes each */
MZ_DEV int32_t mz_bz_byte(mz_bz_bits *B, mz_bz_lds *S) {
    MZ_LANE_DECL
    if (B->pos >= B->in_len) return -1;
    if (B->pos - B->base >= MZ_BZ_INBUF) {
        B->base = B->pos;
        MZ_WAVE_SYNC();
        MZ_LANES {
            const uint32_t o = B->base + 4u * (uint32_t)lane;
            if (o + 4u <= B->in_len && o + 4u > o) {
                mz_st4(&S->inbuf[4 * lane], mz_ld4(B->in + o));
            } else {
                for (uint32_t k = 0; k < 4u; k++)
                    if (o + k < B->in_len) S->inbuf[4u * (uint32_t)lane + k] = B->in[o + k];
            }
        }
        MZ_WAVE_SYNC();
    }
    const uint32_t b = MZ_UNIFORM(S->inbuf[B->pos - B->base]);
    B->pos++;
    return (int32_t)b;
}

#define MZ_BZ_FAIL(code)  \
    do {                  \
        st = (code);      \
        goto done;        \
    } while (0)
/* n <= 24 bits, MSB first */
#define MZ_BZ_GET(var, n)                                              \
    do {                                                               \
        while (B.cnt < (uint32_t)(n)) {                                \
            const int32_t _b = mz_bz_byte(&B, S);                      \
            if (_b < 0) MZ_BZ_FAIL(MZHIP_BUF_ERROR);                   \
            B.acc = (B.acc << 8) | (uint32_t)_b;                       \
            B.cnt += 8u;                                               \
        }                                                              \
        B.cnt -= (uint32_t)(n);                                        \
        (var) = (B.acc >> B.cnt) & ((1u << (n)) - 1u);                 \
    } while (0)
#define MZ_BZ_EXPECT(byte)                                   \
    do {                                                     \
        MZ_BZ_GET(u, 8);                                     \
        if (u != (byte)) MZ_BZ_FAIL(MZHIP_DATA_ERROR);       \
    } while (0)
/* GET_MTF_VAL of libbz2: the selector step every 50 symbols, then minLen bits and one more while the value exceeds limit[len] */
#define MZ_BZ_SYM(sym)                                                                   \
    do {                                                                                 \
        if (group_pos == 0) {                                                            \
            group_no++;                                                                  \
            if (group_no >= n_sel) MZ_BZ_FAIL(MZHIP_DATA_ERROR);                         \
            group_pos = 50;                                                              \
            g = MZ_UNIFORM(sel[group_no]);                                               \
            g_min = MZ_UNIFORM(S->minlen[g]);                                            \
        }                                                                                \
        group_pos--;                                                                     \
        zn = g_min;                                                                      \
        MZ_BZ_GET(zvec, zn);                                                             \
        for (;;) {                                                                       \
            if (zn > 20u) MZ_BZ_FAIL(MZHIP_DATA_ERROR);                                  \
            if ((int32_t)zvec <= (int32_t)MZ_UNIFORM(S->limit[g][zn])) break;            \
            zn++;                                                                        \
            MZ_BZ_GET(u, 1);                                                             \
            zvec = (zvec << 1) | u;                                                      \
        }                                                                                \
        zvec -= MZ_UNIFORM(S->base[g][zn]);                                              \
        if (zvec >= MZ_BZ_ALPHA) MZ_BZ_FAIL(MZHIP_DATA_ERROR);                           \
        (sym) = MZ_UNIFORM(S->perm[g][zvec]);                                            \
    } while (0)

MZ_DEV void mz_bzip2_entry(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, mz_bz_lds *S, const uint32_t *crc_tab,
                           const mzhip_crc_tables *tabs, uint8_t *scratch, mz_bz_result *res) {
    MZ_LANE_DECL
    MZ_BZPROF_DECL
    uint32_t *const tt = (uint32_t *)scratch;
    uint8_t *const lb = scratch + MZ_BZ_L_OFF;
    uint8_t *const sel = scratch + MZ_BZ_SEL_OFF;
    mz_bz_bits B;
    int32_t st = MZHIP_DATA_ERROR;
    uint32_t u = 0, level = 0, o = 0, o_good = 0, combined = 0, stored = 0, orig = 0, n_in_use = 0, alpha = 0, n_groups = 0, n_sel = 0;
    uint32_t used16 = 0, sel_mtf = 0, nblock = 0, nblock_max = 0, group_no = 0, group_pos = 0, g = 0, g_min = 0, zn = 0, zvec = 0;
    uint32_t sym = 0, eob = 0, bcrc = 0, p = 0, prev = 0, cnt4 = 0, crc = 0;
    B.in = in;
    B.in_len = in_len;
    B.pos = 0;
    B.base = 0u - MZ_BZ_INBUF;
    B.acc = 0;
    B.cnt = 0;

    MZ_LANES { /* the block CRC's table: MSB-first, polynomial 0x04C11DB7 */
        for (uint32_t k = 0; k < 4u; k++) {
            uint32_t c = (4u * (uint32_t)lane + k) << 24;
            for (int b = 0; b < 8; b++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
            S->bzcrc[4u * (uint32_t)lane + k] = c;
        }
    }
    MZ_WAVE_SYNC();

    MZ_BZ_EXPECT(0x42u); /* "BZh" */
    MZ_BZ_EXPECT(0x5Au);
    MZ_BZ_EXPECT(0x68u);
    MZ_BZ_GET(level, 8);
    if (level < 0x31u || level > 0x39u) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
    level -= 0x30u;
    nblock_max = 100000u * level;

    for (;;) {
        MZ_BZ_GET(u, 8);
        if (u == 0x17u) { /* the stream's end: 0x177245385090, then the combined CRC */
            MZ_BZ_EXPECT(0x72u);
            MZ_BZ_EXPECT(0x45u);
            MZ_BZ_EXPECT(0x38u);
            MZ_BZ_EXPECT(0x50u);
            MZ_BZ_EXPECT(0x90u);
            stored = 0;
            for (int k = 0; k < 4; k++) {
                MZ_BZ_GET(u, 8);
                stored = (stored << 8) | u;
            }
            if (stored != combined) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
            st = MZHIP_OK;
            break;
        }
        if (u != 0x31u) MZ_BZ_FAIL(MZHIP_DATA_ERROR); /* a block: 0x314159265359 */
        MZ_BZ_EXPECT(0x41u);
        MZ_BZ_EXPECT(0x59u);
        MZ_BZ_EXPECT(0x26u);
        MZ_BZ_EXPECT(0x53u);
        MZ_BZ_EXPECT(0x59u);
        stored = 0;
        for (int k = 0; k < 4; k++) {
            MZ_BZ_GET(u, 8);
            stored = (stored << 8) | u;
        }
        MZ_BZ_GET(u, 1);
        if (u) MZ_BZ_FAIL(MZHIP_UNSUPPORTED); /* randomised: no compressor has written it since 0.9.5 */
        orig = 0;
        for (int k = 0; k < 3; k++) {
            MZ_BZ_GET(u, 8);
            orig = (orig << 8) | u;
        }
        if (orig > 10u + nblock_max) MZ_BZ_FAIL(MZHIP_DATA_ERROR);

        /* ---- symbol map */
        MZ_BZ_GET(used16, 16);
        n_in_use = 0;
        for (uint32_t i = 0; i < 16u; i++) {
            if (!((used16 >> (15u - i)) & 1u)) continue;
            MZ_BZ_GET(u, 16);
            for (uint32_t j = 0; j < 16u; j++)
                if ((u >> (15u - j)) & 1u) {
                    S->seq2unseq[n_in_use] = (uint8_t)(16u * i + j);
                    n_in_use++;
                }
        }
        if (n_in_use == 0) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
        alpha = n_in_use + 2u;

        /* ---- selectors, their move-to-front undone as they come (the list: six nibbles of one word) */
        MZ_BZ_GET(n_groups, 3);
        if (n_groups < 2u || n_groups > MZ_BZ_GROUPS) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
        MZ_BZ_GET(n_sel, 15);
        if (n_sel < 1u) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
        sel_mtf = 0x543210u;
        for (uint32_t i = 0; i < n_sel; i++) {
            uint32_t j = 0;
            for (;;) {
                MZ_BZ_GET(u, 1);
                if (!u) break;
                j++;
                if (j >= n_groups) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
            }
            if (i < MZ_BZ_MAX_SELECTORS) { /* libbz2 1.0.8 reads and drops the selectors behind 18 002 */
                const uint32_t v = (sel_mtf >> (4u * j)) & 15u;
                const uint32_t low = sel_mtf & ((1u << (4u * j)) - 1u);
                sel_mtf = (sel_mtf & ~((1u << (4u * j + 4u)) - 1u)) | (low << 4) | v;
                sel[i] = (uint8_t)v; /* wave-uniform: stored by all lanes (same address, same value) */
            }
        }
        if (n_sel > MZ_BZ_MAX_SELECTORS) n_sel = MZ_BZ_MAX_SELECTORS;

        /* ---- code lengths */
        for (uint32_t t = 0; t < n_groups; t++) {
            uint32_t curr;
            MZ_BZ_GET(curr, 5);
            for (uint32_t i = 0; i < alpha; i++) {
                for (;;) {
                    if (curr < 1u || curr > 20u) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
                    MZ_BZ_GET(u, 1);
                    if (!u) break;
                    MZ_BZ_GET(u, 1);
                    curr = u ? curr - 1u : curr + 1u;
                }
                S->len[t][i] = (uint8_t)curr;
            }
        }

        /* ---- limit / base / perm per table, as BZ2_hbCreateDecodeTables computes them (complete set or not) */
        MZ_WAVE_SYNC();
        for (uint32_t t = 0; t < n_groups; t++) {
            uint32_t min_len = 32u, max_len = 0u;
            int32_t vec = 0;
            MZ_LANES {
                if (lane < (int)MZ_BZ_LENS) {
                    S->limit[t][lane] = 0;
                    S->base[t][lane] = 0;
                }
            }
            MZ_WAVE_SYNC();
            MZ_LANES {
                for (uint32_t i = (uint32_t)lane; i < alpha; i += 64u) MZ_LDS_ATOMIC_INC((uint32_t *)&S->base[t][S->len[t][i] + 1u]);
            }
            MZ_WAVE_SYNC();
            for (uint32_t i = 1; i <= 20u; i++)
                if (MZ_UNIFORM((uint32_t)S->base[t][i + 1u]) != 0u) {
                    if (min_len > i) min_len = i;
                    max_len = i;
                }
            for (uint32_t i = 1; i < 23u; i++) S->base[t][i] = (int32_t)MZ_UNIFORM((uint32_t)(S->base[t][i] + S->base[t][i - 1u]));
            MZ_WAVE_SYNC();
            MZ_LANES { /* canonical order: by length, then by symbol index */
                for (uint32_t i = (uint32_t)lane; i < alpha; i += 64u) {
                    const uint32_t l = S->len[t][i];
                    uint32_t c = 0;
                    for (uint32_t j = 0; j < i; j++) c += S->len[t][j] == l;
                    S->perm[t][(uint32_t)S->base[t][l] + c] = (uint16_t)i;
                }
            }
            MZ_WAVE_SYNC();
            for (uint32_t i = min_len; i <= max_len; i++) {
                vec += (int32_t)MZ_UNIFORM((uint32_t)(S->base[t][i + 1u] - S->base[t][i]));
                S->limit[t][i] = vec - 1;
                vec <<= 1;
            }
            for (uint32_t i = min_len + 1u; i <= max_len; i++)
                S->base[t][i] = (int32_t)MZ_UNIFORM((uint32_t)(((S->limit[t][i - 1u] + 1) << 1) - S->base[t][i]));
            S->minlen[t] = (uint8_t)min_len;
            MZ_WAVE_SYNC();
        }

        /* ---- the symbol loop */
        MZ_LANES {
            for (uint32_t k = 0; k < 4u; k++) {
                S->mtf[4u * (uint32_t)lane + k] = (uint8_t)(4u * (uint32_t)lane + k);
                S->unzftab[4u * (uint32_t)lane + k] = 0;
            }
        }
        MZ_WAVE_SYNC();
        eob = n_in_use + 1u;
        group_no = 0xFFFFFFFFu;
        group_pos = 0;
        nblock = 0;
        MZ_BZ_SYM(sym);
        while (sym != eob) {
            if (sym <= 1u) { /* RUNA / RUNB: a run of the byte at the list's front */
                uint32_t es = 0, weight = 1, uc;
                do {
                    if (weight >= 2u * 1024u * 1024u) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
                    es += weight << sym;
                    weight <<= 1;
                    MZ_BZ_SYM(sym);
                } while (sym <= 1u);
                uc = MZ_UNIFORM(S->seq2unseq[MZ_UNIFORM(S->mtf[0])]);
                if (es > nblock_max - nblock) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
                S->unzftab[uc] = MZ_UNIFORM(S->unzftab[uc]) + es;
                MZ_LANES {
                    for (uint32_t k = (uint32_t)lane; k < es; k += 64u) lb[nblock + k] = (uint8_t)uc;
                }
                nblock += es;
            } else {
                const uint32_t nn = sym - 1u;
                uint32_t uc, b;
                if (nblock >= nblock_max) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
                uc = MZ_UNIFORM(S->mtf[nn]);
                /* the list moves up by one in front of nn, the highest 64 positions first */
                for (uint32_t k0 = (nn - 1u) & ~63u;; k0 -= 64u) {
                    PV(uint32_t, v);
                    MZ_LANES {
                        const uint32_t j = k0 + (uint32_t)lane;
                        P(v) = j < nn ? S->mtf[j] : 0u;
                    }
                    MZ_WAVE_SYNC();
                    MZ_LANES {
                        const uint32_t j = k0 + (uint32_t)lane;
                        if (j < nn) S->mtf[j + 1u] = (uint8_t)P(v);
                    }
                    MZ_WAVE_SYNC();
                    if (k0 == 0) break;
                }
                S->mtf[0] = (uint8_t)uc;
                b = MZ_UNIFORM(S->seq2unseq[uc]);
                S->unzftab[b] = MZ_UNIFORM(S->unzftab[b]) + 1u;
                lb[nblock] = (uint8_t)b; /* wave-uniform store */
                nblock++;
                MZ_BZ_SYM(sym);
            }
        }
        if (orig >= nblock) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
        MZ_BZPROF_MARK(0);

        /* ---- where each byte value starts in the sorted column: 4 values per lane, one scan across the wave */
        MZ_WAVE_SYNC();
        {
            PV(uint32_t, tot);
            PV(uint32_t, incl);
            MZ_LANES {
                const uint32_t *q = &S->unzftab[4u * (uint32_t)lane];
                P(tot) = q[0] + q[1] + q[2] + q[3];
            }
            MZ_INCL_SCAN(incl, tot);
            MZ_LANES {
                const uint32_t *q = &S->unzftab[4u * (uint32_t)lane];
                uint32_t e = P(incl) - P(tot);
                for (uint32_t k = 0; k < 4u; k++) {
                    S->cftab[4u * (uint32_t)lane + k] = e;
                    e += q[k];
                }
            }
        }
        MZ_CHASE_FENCE(); /* the block's bytes were stored through one address per step and are read a lane per position */
        MZ_WAVE_SYNC();

        /* ---- the links: a stable counting sort, 64 positions per step */
        for (uint32_t i0 = 0; i0 < nblock; i0 += 64u) {
            PV(uint32_t, byt);
            uint64_t valid, bal[8];
            MZ_LANES {
                const uint32_t i = i0 + (uint32_t)lane;
                P(byt) = i < nblock ? lb[i] : 0u;
            }
            MZ_BALLOT(valid, i0 + (uint32_t)lane < nblock);
            MZ_BALLOT(bal[0], P(byt) & 1u);
            MZ_BALLOT(bal[1], P(byt) & 2u);
            MZ_BALLOT(bal[2], P(byt) & 4u);
            MZ_BALLOT(bal[3], P(byt) & 8u);
            MZ_BALLOT(bal[4], P(byt) & 16u);
            MZ_BALLOT(bal[5], P(byt) & 32u);
            MZ_BALLOT(bal[6], P(byt) & 64u);
            MZ_BALLOT(bal[7], P(byt) & 128u);
            PV(uint32_t, last); /* this lane is the highest one of its byte value: it moves cftab on */
            PV(uint32_t, same);
            MZ_LANES {
                const uint32_t i = i0 + (uint32_t)lane, b = P(byt);
                uint64_t m = valid;
                for (uint32_t k = 0; k < 8u; k++) m &= ((b >> k) & 1u) ? bal[k] : ~bal[k];
                const uint32_t rank = MZ_RANK_BELOW(m), n_same = mz_popc64(m);
                P(last) = 0;
                P(same) = n_same;
                if (i < nblock) {
                    const uint32_t slot = S->cftab[b] + rank; /* < nblock: the counts sum to nblock */
                    tt[slot] = (i << 8) | b;
                    P(last) = rank + 1u == n_same;
                }
            }
            MZ_WAVE_SYNC();
            MZ_LANES {
                if (P(last)) S->cftab[P(byt)] += P(same);
            }
            MZ_WAVE_SYNC();
        }
        MZ_CHASE_FENCE();
        MZ_WAVE_SYNC();
        MZ_BZPROF_MARK(1);

        /* ---- the chain walk, the final run-length stage undone on the way: after four equal bytes the next is a count */
        p = orig;
        prev = 256u;
        cnt4 = 0;
        bcrc = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < nblock; i++) {
            const uint32_t v = MZ_UNIFORM(tt[p]), c = v & 255u;
            p = v >> 8;
            if (cnt4 == 4u) {
                if (c > out_cap - o) MZ_BZ_FAIL(MZHIP_OUT_FULL);
                MZ_LANES {
                    for (uint32_t k = (uint32_t)lane; k < c; k += 64u) out[o + k] = (uint8_t)prev;
                }
                for (uint32_t k = 0; k < c; k++) bcrc = (bcrc << 8) ^ MZ_UNIFORM(S->bzcrc[(bcrc >> 24) ^ prev]);
                o += c;
                prev = 256u;
                cnt4 = 0;
                continue;
            }
            if (c == prev) {
                cnt4++;
            } else {
                prev = c;
                cnt4 = 1;
            }
            if (o >= out_cap) MZ_BZ_FAIL(MZHIP_OUT_FULL);
            out[o] = (uint8_t)c; /* wave-uniform store */
            o++;
            bcrc = (bcrc << 8) ^ MZ_UNIFORM(S->bzcrc[(bcrc >> 24) ^ c]);
        }
        if (cnt4 == 4u) MZ_BZ_FAIL(MZHIP_DATA_ERROR); /* libbz2 takes a count from behind the block's end and then calls the block corrupt */
        bcrc = ~bcrc;
        if (bcrc != stored) MZ_BZ_FAIL(MZHIP_DATA_ERROR);
        combined = ((combined << 1) | (combined >> 31)) ^ bcrc;
        o_good = o;
        MZ_BZPROF_MARK(2);
    }

done:
    /* the ZIP CRC-32 of what stands: the K2 fold over the finished bytes */
    MZ_CHASE_FENCE();
    MZ_WAVE_SYNC();
    {
        PV(uint32_t, acc);
        PV(uint32_t, tmp);
        uint32_t folded = 0;
        MZ_LANES { P(acc) = (lane == 0) ? 0xFFFFFFFFu : 0u; }
        MZ_CRC_FOLD_TILES(acc, folded, out, o_good, crc_tab, tabs->kx);
        MZ_CRC_FINISH(crc, acc, tmp, folded, out, o_good, crc_tab, tabs);
    }
    MZ_BZPROF_MARK(3);
    MZ_BZPROF_FLUSH
    res->out_len = o_good;
    res->in_used = B.pos;
    res->crc = crc;
    res->status = st;
}

#endif
