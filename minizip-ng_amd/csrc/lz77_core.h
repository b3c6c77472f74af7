/* lz77_core.h -- the LZ77 step that the DEFLATE encoder (K4, deflate_core.h mz_deflate_piece) and the LZMA tokenizer (K6,
 * lzma_enc_core.h mz_lz_tokenize) share: 64 positions per step, one per lane.  Every parse rule the two have in common is
 * written here, or in lz77_select.inc (the pointer-doubling selection), and nowhere else:
 *   - the hash of a position's four bytes and the per-wave bucket tables: way 0 = head[hash] (LDS), ways 1.. =
 *     xhead[(w - 1) << MZ_DEF_HBITS | hash] (extra LDS behind the wave's struct, may be NULL for one way); every entry is
 *     the low 16 bits of a position, newest in way 0;
 *   - a position inherits a longer match from the lanes 1 and 2 below;
 *   - the lazy rule, and the successor word the selection starts from.
 * What differs stays with its encoder: how the candidates of a bucket are measured (K4 prefetches sixteen bytes one step
 * ahead and bounds a match by its window; K6 bounds it by the dictionary and walks the far links), K4's warm-up of one
 * way, and what becomes of the selected tokens.
 * Macros where per-lane variables (PV / P(), wave.h) cross, because the same text is the gfx950 kernel and the host
 * emulation.  The hash and the clear are macros as well although only values cross: as inlined functions they leave the
 * kernels' results alone but not their code (the tokenizer's history loop gains a compare; the clear's loops renumber the
 * jump targets clang counts per function, which K4's exits keep as immediates).  A token word: [8:0] match length (0 = literal), the distance or
 * the literal byte from bit 9 up. */
#ifndef MZHIP_LZ77_CORE_H
#define MZHIP_LZ77_CORE_H

#include "wave.h"

#ifndef MZ_DEF_HBITS
#define MZ_DEF_HBITS 12
#endif
#define MZ_DEF_MINMATCH 4u
#define MZ_DEF_WAYS_BEST 4u /* the deepest bucket: the default class of either encoder (the fast class keeps one way) */

/* the bucket of a position: a hash of its four bytes */
#define MZ_LZ_HASH4(v) (((v) * 2654435761u) >> (32 - MZ_DEF_HBITS))

/* empty buckets, two entries per word (inside MZ_LANES) */
#define MZ_LZ_CLEAR(head, xhead, ways)                                                                                 \
    for (uint32_t i = (uint32_t)lane; i < (1u << MZ_DEF_HBITS) / 2u; i += 64u) ((uint32_t *)(head))[i] = 0u;           \
    for (uint32_t i = (uint32_t)lane; i < ((ways) - 1u) * ((1u << MZ_DEF_HBITS) / 2u); i += 64u) ((uint32_t *)(xhead))[i] = 0u;

/* bucket h as it stands into P(c0) (way 0, where ok0) and P(cx)[] (the ways 1.. that are kept, where ok); zeros elsewhere
 * (inside MZ_LANES) */
#define MZ_LZ_BUCKET_READ(head, xhead, ways, h, ok0, ok, c0, cx)                                                       \
    P(c0) = (ok0) ? (uint32_t)(head)[h] : 0u;                                                                          \
    for (uint32_t w = 1; w < MZ_DEF_WAYS_BEST; w++)                                                                    \
        P(cx)[w - 1u] = ((ok) && w < (ways)) ? (uint32_t)(xhead)[((w - 1u) << MZ_DEF_HBITS) | (h)] : 0u;

/* pos enters bucket h, whose entries as read above move down one way: lanes that share a bucket write the same older
 * entries, one of them wins way 0 (inside MZ_LANES, a MZ_WAVE_SYNC() behind the read) */
#define MZ_LZ_BUCKET_PUSH(head, xhead, ways, h, pos, c0, cx)                                                           \
    for (uint32_t w = MZ_DEF_WAYS_BEST - 1u; w >= 1u; w--)                                                             \
        if (w < (ways)) (xhead)[((w - 1u) << MZ_DEF_HBITS) | (h)] = (uint16_t)(w == 1u ? P(c0) : P(cx)[w - 2u]);       \
    (head)[h] = (uint16_t)(pos);

/* A match of length L at position q is a match of length L - k at q + k, same distance: a position whose own bucket had
 * lost that candidate inherits it from the lanes 1 and 2 (then up to 3) below -- worth 1.2 % of DEFLATE's output under the
 * lazy rule (tests/study/enc_parse.c INH=3).  P(pk) = every position's match, nv = valid positions of the step. */
#define MZ_LZ_INHERIT(pk, nv, ways)                                                                                    \
    if ((ways) > 1u) {                                                                                                 \
        for (uint32_t sh = 1u; sh <= 2u; sh <<= 1) {                                                                   \
            PV(uint32_t, pin);                                                                                         \
            MZ_GATHER4(pin, pk, 4u * (((uint32_t)lane - sh) & 63u));                                                   \
            MZ_LANES {                                                                                                 \
                const uint32_t il = P(pin) & 511u;                                                                     \
                if ((uint32_t)lane >= sh && (uint32_t)lane < (nv) && il >= MZ_DEF_MINMATCH + sh && il - sh > (P(pk) & 511u)) \
                    P(pk) = (il - sh) | (P(pin) & ~511u);                                                              \
            }                                                                                                          \
        }                                                                                                              \
    }

/* the successor word of a lane whose token is mlen long (0 = a literal): 4 * successor lane; bit 12 set: terminal (the
 * successor lies beyond the step's nv positions) */
MZ_DEV uint32_t mz_lz_succ(uint32_t lane, uint32_t mlen, uint32_t nv) {
    const uint32_t nx = lane + (mlen ? mlen : 1u);
    return (lane >= nv || nx >= nv) ? (0x1000u | (4u * nx)) : (4u * nx);
}

/* Lazy evaluation (what zlib does from level 4 up): a match yields to a longer one starting at the next position -- this
 * position then goes out as a literal, P(lit); the default class also looks two positions ahead (two literals must buy
 * more than one byte).  Leaves P(pk) = every position's token and P(g1) = its successor word. */
#define MZ_LZ_LAZY(pk, lit, g1, nv, ways)                                                                              \
    PV(uint32_t, pkn);                                                                                                 \
    PV(uint32_t, pkn2);                                                                                                \
    MZ_GATHER4(pkn, pk, 4u * ((uint32_t)lane + 1u));                                                                   \
    MZ_GATHER4(pkn2, pk, 4u * ((uint32_t)lane + 2u));                                                                  \
    MZ_LANES {                                                                                                         \
        uint32_t mlen = P(pk) & 511u;                                                                                  \
        if (mlen && (uint32_t)lane + 1u < (nv) && (P(pkn) & 511u) > mlen) mlen = 0u;                                   \
        if ((ways) > 1u && mlen && (uint32_t)lane + 2u < (nv) && (P(pkn2) & 511u) > mlen + 1u) mlen = 0u;              \
        P(pk) = mlen ? P(pk) : (P(lit) << 9);                                                                          \
        P(g1) = mz_lz_succ((uint32_t)lane, mlen, nv);                                                                  \
    }

#endif
