/* zstd_core.h -- one Zstandard entry (ZIP method 93: one or more frames of RFC 8878, skippable frames among them) decoded by
 * one wave.
 *
 * Written in the wave.h vocabulary: the same text is the gfx950 kernel body (k_zstd_batch) and, under
 * g++ -DMZHIP_HOST_EMUL, the host build the CPU tests run (tests/emul/emul_zstd.cpp).  ZSTD_decompress of libzstd is the
 * model for what is accepted and in which order problems are met; where this reader is stricter than libzstd 1.4.8 (the
 * block size is held to min(Window_Size, 128 KiB), the reserved bits of the sequence modes must be 0, a Huffman code is at
 * most 11 bits long, a repeat offset that resolves to 0 is an error) it follows the format's text.
 *
 * Per block a wave
 *   1. parses the block header, the literals header and the table descriptions wave-uniform; the input is read at BYTE
 *      granularity through a 256-byte LDS window that the lanes fill, never outside [in, in + in_len);
 *   2. builds the Huffman decode table (at most 11 bits, 2 048 cells) with a lane per symbol: the weights are ranked, a
 *      prefix over the ranks gives each weight its first cell, a symbol's lane writes its cells.  The FSE decode tables
 *      (literal lengths, offsets, match lengths, Huffman weights) are spread and numbered wave-uniform;
 *   3. decodes the literal streams, a lane per stream (four lanes, or one), into the wave's scratch in HBM: 128 KiB of
 *      literals do not fit LDS at 8 single-wave workgroups per CU.  Raw and RLE literals are copied / filled by all lanes;
 *   4. runs the three-state FSE machine over the backward bitstream, wave-uniform; repeat offsets are resolved there, so
 *      every sequence is (literal length, match length, absolute distance) when it is executed;
 *   5. executes each sequence with all lanes: the literal run and the match are written in ONE pass, byte k of the match
 *      reads out[start - D + (k mod D)] when D < match length (every source byte then lies in front of the match, so the
 *      lanes do not depend on each other), and a source byte that falls into the literal run just being written is taken
 *      from the literals instead.  One fence per sequence orders it behind the stores of the sequences before it;
 *   6. at a frame's end folds XXH64 over the frame's bytes on four lanes, one accumulator each, and after the last frame
 *      the ZIP CRC-32 over everything with the K2 tiles.
 *
 * LDS: sizeof(mz_zs_lds) = 10 304 bytes per wave.  Scratch in HBM per wave: MZ_ZS_SCRATCH_BYTES = 131 328 (the literals of one
 * block, 128 KiB, and a 256-byte margin); sequences are executed as they are decoded and never spilled.
 */
#ifndef MZHIP_ZSTD_CORE_H
#define MZHIP_ZSTD_CORE_H

#include "crc32_core.h"
#include "wave.h"

#define MZ_ZS_BLOCK_MAX 131072u
#define MZ_ZS_SCRATCH_BYTES 131328u /* MZ_ZS_BLOCK_MAX + 256 */
#define MZ_ZS_INBUF 256u
#define MZ_ZS_HUF_LOG_MAX 11u
#define MZ_ZS_ERR 0xFFFFFFFFu

/* a decode cell of an FSE table: symbol | bits to read << 8 | baseline of the next state << 16 */
typedef struct mz_zs_lds {
    uint32_t ll[512];
    uint32_t ml[512];
    uint32_t of[256];
    uint32_t wt[64];    /* the FSE table of compressed Huffman weights (accuracy log <= 6) */
    uint16_t huf[2048]; /* symbol | code length << 8, indexed by the next huf_log bits */
    int16_t norm[64];   /* the normalised counts of the table being built */
    uint16_t next[64];
    uint32_t rank[16];
    uint8_t weights[256];
    uint8_t inbuf[MZ_ZS_INBUF];
} mz_zs_lds;

typedef struct mz_zs_result {
    uint32_t out_len; /* status 0: the bytes of all frames; otherwise the bytes of the complete blocks in front of the problem */
    uint32_t in_used; /* status 0: in_len */
    uint32_t crc;     /* CRC-32 of out[0 .. out_len) */
    int32_t status;
} mz_zs_result;

typedef struct mz_zs_ctx {
    const uint8_t *in;
    uint32_t in_len;
    uint32_t base; /* offset of inbuf[0] in the input */
    uint8_t *out;
    uint32_t out_cap;
    uint8_t *lit;
    uint32_t o;       /* bytes written */
    uint32_t fo;      /* where the frame's output starts */
    uint32_t blk_max; /* min(Window_Size, 128 KiB) */
    uint32_t rep0, rep1, rep2;
    uint32_t have_huf, huf_log; /* a tree from an earlier block of this frame stands in S->huf */
    uint32_t have_seq;          /* an earlier block of this frame had sequences: "repeat" has tables to repeat */
    uint32_t al_ll, al_of, al_ml;
#if defined(MZ_PROF) && !defined(MZHIP_HOST_EMUL)
    uint32_t prof_acc;
    uint64_t prof_t0;
#endif
} mz_zs_ctx;

/* the backward bitstream: bits [0, bits) of bytes [start, start + n) are still unread, the highest first */
typedef struct mz_zs_bits {
    uint32_t start, n;
    int32_t bits;  /* negative: more was read than there is */
    int32_t acc_b; /* acc holds the bytes acc_b .. acc_b + 7 of the stream (zeros outside it) */
    uint64_t acc;
    uint32_t cached;
} mz_zs_bits;

/* measurement builds (make PROF=1): cycles of the stages, summed over all waves, in mz_prof_buf[23 .. 27]:
 * 23 headers + tables, 24 literal streams, 25 sequence decode, 26 execution (literal and match copies), 27 XXH64 + CRC-32 */
#if defined(MZ_PROF) && !defined(MZHIP_HOST_EMUL)
#define MZ_ZSPROF_INIT(C) do { (C)->prof_acc = 0; (C)->prof_t0 = __builtin_readcyclecounter(); } while (0)
#define MZ_ZSPROF_MARK(C, i)                                                            \
    do {                                                                                \
        const uint32_t _pd = (uint32_t)(__builtin_readcyclecounter() - (C)->prof_t0);   \
        (C)->prof_acc += (lane == 23 + (i)) ? _pd : 0u;                                 \
        (C)->prof_t0 = __builtin_readcyclecounter();                                    \
    } while (0)
#define MZ_ZSPROF_FLUSH(C) if (lane >= 23 && lane < 28) atomicAdd(&mz_prof_buf[lane], (unsigned long long)(C)->prof_acc);
#else
#define MZ_ZSPROF_INIT(C) ((void)0)
#define MZ_ZSPROF_MARK(C, i) ((void)0)
#define MZ_ZSPROF_FLUSH(C)
#endif

/* counters of the host emulation (-DMZ_ZS_STATS): the tests hold each program family to its name with them */
#if defined(MZ_ZS_STATS) && defined(MZHIP_HOST_EMUL)
typedef struct mz_zs_stats {
    uint32_t lit[16];     /* literals type * 4 + size format */
    uint32_t mode[3][4];  /* LL / OF / ML table x mode */
    uint32_t ll_code[36], ml_code[53], of_code[32];
    uint32_t rep_rule[7]; /* 0 a new offset; 1 - 3 offset value 1 - 3 with literals; 4 - 6 the same with literal length 0 */
    uint32_t overlap[72]; /* the match was longer than its distance (distances 1 .. 70; 71: any longer one) */
    uint32_t weights_direct, weights_fse, streams1, streams4, treeless, frames, skippable, checksums;
    uint32_t less_than_one, zero_repeat3;
} mz_zs_stats;
static mz_zs_stats mz_zs_stat;
#define MZ_ZS_STAT(x) (x)
#else
#define MZ_ZS_STAT(x) ((void)0)
#endif

MZ_DEV uint32_t mz_zs_highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); } /* v != 0 */

/* the input byte at pos (< in_len); the LDS window is refilled by the lanes, 4 bytes each, at a multiple of 256 */
MZ_DEV uint32_t mz_zs_byte(mz_zs_ctx *C, mz_zs_lds *S, uint32_t pos) {
    MZ_LANE_DECL
    if (pos - C->base >= MZ_ZS_INBUF) {
        C->base = pos & ~(MZ_ZS_INBUF - 1u);
        MZ_WAVE_SYNC();
        MZ_LANES {
            const uint32_t o = C->base + 4u * (uint32_t)lane;
            if (o + 4u <= C->in_len && o + 4u > o) {
                mz_st4(&S->inbuf[4 * lane], mz_ld4(C->in + o));
            } else {
                for (uint32_t k = 0; k < 4u; k++)
                    if (o + k < C->in_len && o + k >= o) S->inbuf[4u * (uint32_t)lane + k] = C->in[o + k];
            }
        }
        MZ_WAVE_SYNC();
    }
    return MZ_UNIFORM(S->inbuf[pos - C->base]);
}

/* n <= 4 bytes, little-endian, at pos (all inside the input) */
MZ_DEV uint32_t mz_zs_le(mz_zs_ctx *C, mz_zs_lds *S, uint32_t pos, uint32_t n) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= mz_zs_byte(C, S, pos + k) << (8u * k);
    return v;
}

/* nb <= 16 bits of a FORWARD bit field (LSB first) that starts at byte p0; bytes at and behind `end` read as 0 */
MZ_DEV uint32_t mz_zs_fbits(mz_zs_ctx *C, mz_zs_lds *S, uint32_t p0, uint32_t end, uint32_t bitpos, uint32_t nb) {
    const uint32_t b = p0 + (bitpos >> 3);
    uint32_t v = 0;
    for (uint32_t j = 0; j < 3u; j++)
        if (b + j < end && b + j >= p0) v |= mz_zs_byte(C, S, b + j) << (8u * j);
    return (v >> (bitpos & 7u)) & ((1u << nb) - 1u);
}

/* opens the backward bitstream [start, start + n): 0 if it is empty or its last byte is 0 (no final-bit marker) */
MZ_DEV uint32_t mz_zs_bits_open(mz_zs_ctx *C, mz_zs_lds *S, mz_zs_bits *B, uint32_t start, uint32_t n) {
    uint32_t last;
    B->start = start;
    B->n = n;
    B->bits = 0;
    B->acc = 0;
    B->acc_b = 0;
    B->cached = 0;
    if (n == 0) return 0;
    last = mz_zs_byte(C, S, start + n - 1u);
    if (last == 0) return 0;
    B->bits = (int32_t)(8u * (n - 1u) + mz_zs_highbit(last));
    return 1;
}

/* the next nb <= 32 bits; bits in front of the stream's first read as 0 and leave B->bits negative */
MZ_DEV uint32_t mz_zs_bits_read(mz_zs_ctx *C, mz_zs_lds *S, mz_zs_bits *B, uint32_t nb) {
    if (nb == 0) return 0;
    const int32_t lo = B->bits - (int32_t)nb, top = B->bits - 1;
    B->bits = lo;
    if (top < 0) return 0;
    if (!B->cached || lo < 8 * B->acc_b || top > 8 * B->acc_b + 63) {
        uint64_t a = 0;
        B->acc_b = (top >> 3) - 7;
        for (int32_t j = 0; j < 8; j++) {
            const int32_t idx = B->acc_b + j;
            if (idx >= 0 && (uint32_t)idx < B->n) a |= (uint64_t)mz_zs_byte(C, S, B->start + (uint32_t)idx) << (8 * j);
        }
        B->acc = a;
        B->cached = 1;
    }
    /* lo >= top - 31 >= 8 * (top >> 3) - 31 > 8 * acc_b: the shift is in 0 .. 63 also where lo is negative */
    return (uint32_t)(B->acc >> (uint32_t)(lo - 8 * B->acc_b)) & (nb >= 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u));
}

/* an FSE table description at p (RFC 8878 4.1.1) into S->norm: the accuracy log to *al, the symbols described to *nsym;
 * -> bytes used, or MZ_ZS_ERR */
MZ_DEV uint32_t mz_zs_fse_read(mz_zs_ctx *C, mz_zs_lds *S, uint32_t p, uint32_t end, uint32_t max_al, uint32_t max_sym, uint32_t *al,
                               uint32_t *nsym) {
    uint32_t bp = 4, acc = 0, sym = 0, T, used;
    if (p >= end) return MZ_ZS_ERR;
    *al = mz_zs_fbits(C, S, p, end, 0, 4) + 5u;
    if (*al > max_al) return MZ_ZS_ERR;
    T = 1u << *al;
    while (acc < T && sym <= max_sym) {
        const uint32_t rem1 = T - acc + 1u, nb = mz_zs_highbit(rem1) + 1u, lower = (1u << (nb - 1u)) - 1u, thr = (1u << nb) - 1u - rem1;
        uint32_t val = mz_zs_fbits(C, S, p, end, bp, nb);
        int32_t prob;
        if ((val & lower) < thr) {
            val &= lower;
            bp += nb - 1u;
        } else {
            if (val > lower) val -= thr;
            bp += nb;
        }
        prob = (int32_t)val - 1;
        acc += prob < 0 ? 1u : (uint32_t)prob;
        S->norm[sym] = (int16_t)prob;
        sym++;
        if (prob < 0) MZ_ZS_STAT(mz_zs_stat.less_than_one++);
        if (prob == 0) { /* a 2-bit count of further zeros; 3 means another count follows */
            for (;;) {
                const uint32_t rep = mz_zs_fbits(C, S, p, end, bp, 2);
                bp += 2u;
                for (uint32_t k = 0; k < rep; k++) {
                    if (sym > max_sym) return MZ_ZS_ERR;
                    S->norm[sym] = 0;
                    sym++;
                }
                if (rep != 3u) break;
                MZ_ZS_STAT(mz_zs_stat.zero_repeat3++);
            }
            if (sym > max_sym) return MZ_ZS_ERR; /* the zeros must be followed by a symbol */
        }
    }
    if (acc != T) return MZ_ZS_ERR;
    used = (bp + 7u) >> 3;
    if (used > end - p) return MZ_ZS_ERR;
    *nsym = sym;
    return used;
}

/* the decode table of S->norm[0 .. nsym) at accuracy log al: "less than 1" symbols from the top, the others spread with
 * the step (T >> 1) + (T >> 3) + 3, then every cell numbered in cell order */
MZ_DEV void mz_zs_fse_build(uint32_t *tab, mz_zs_lds *S, uint32_t nsym, uint32_t al) {
    const uint32_t T = 1u << al, mask = T - 1u, step = (T >> 1) + (T >> 3) + 3u;
    uint32_t high = T - 1u, pos = 0;
    MZ_WAVE_SYNC();
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t pr = (int32_t)(int16_t)MZ_UNIFORM((uint32_t)(int32_t)S->norm[s]);
        if (pr < 0) {
            tab[high] = s;
            high--;
            S->next[s] = 1;
        } else {
            S->next[s] = (uint16_t)pr;
        }
    }
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t pr = (int32_t)(int16_t)MZ_UNIFORM((uint32_t)(int32_t)S->norm[s]);
        for (int32_t i = 0; i < pr; i++) {
            tab[pos] = s;
            do pos = (pos + step) & mask;
            while (pos > high && high != 0xFFFFFFFFu);
        }
    }
    MZ_WAVE_SYNC();
    for (uint32_t u = 0; u < T; u++) {
        const uint32_t s = MZ_UNIFORM(tab[u]) & 63u, x = MZ_UNIFORM(S->next[s]);
        const uint32_t nb = al - mz_zs_highbit(x | 1u);
        S->next[s] = (uint16_t)(x + 1u);
        tab[u] = s | (nb << 8) | ((((x << nb) - T) & 0xFFFFu) << 16);
    }
    MZ_WAVE_SYNC();
}

/* a table of one cell that reads no bits: RLE mode */
MZ_DEV void mz_zs_fse_rle(uint32_t *tab, uint32_t sym) {
    MZ_WAVE_SYNC();
    tab[0] = sym;
    MZ_WAVE_SYNC();
}

#if defined(MZHIP_HOST_EMUL)
#define MZ_ZS_TABLE static const
#else
#define MZ_ZS_TABLE __device__ __constant__ static const
#endif
/* the predefined distributions (RFC 8878 3.1.1.3.2.2), accuracy logs 6, 6 and 5 */
#define MZ_ZS_LL_DEFAULT {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1}
#define MZ_ZS_ML_DEFAULT {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1}
#define MZ_ZS_OF_DEFAULT {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1}
MZ_ZS_TABLE int8_t mz_zs_dll[36] = MZ_ZS_LL_DEFAULT;
MZ_ZS_TABLE int8_t mz_zs_dml[53] = MZ_ZS_ML_DEFAULT;
MZ_ZS_TABLE int8_t mz_zs_dof[29] = MZ_ZS_OF_DEFAULT;

/* literal-length and match-length codes: baseline and extra bits */
MZ_DEV uint32_t mz_zs_ll_base(uint32_t c, uint32_t *nb) {
    if (c < 16u) { *nb = 0; return c; }
    if (c < 20u) { *nb = 1; return 16u + 2u * (c - 16u); }
    if (c < 22u) { *nb = 2; return 24u + 4u * (c - 20u); }
    if (c < 24u) { *nb = 3; return 32u + 8u * (c - 22u); }
    if (c == 24u) { *nb = 4; return 48u; }
    *nb = c - 19u; /* 25: 6 bits from 64, 26: 7 from 128, ... 35: 16 from 65 536 */
    return 1u << (c - 19u);
}
MZ_DEV uint32_t mz_zs_ml_base(uint32_t c, uint32_t *nb) {
    if (c < 32u) { *nb = 0; return c + 3u; }
    if (c < 36u) { *nb = 1; return 35u + 2u * (c - 32u); }
    if (c < 38u) { *nb = 2; return 43u + 4u * (c - 36u); }
    if (c < 40u) { *nb = 3; return 51u + 8u * (c - 38u); }
    if (c < 42u) { *nb = 4; return 67u + 16u * (c - 40u); }
    if (c == 42u) { *nb = 5; return 99u; }
    *nb = c - 36u; /* 43: 7 bits from 131, 44: 8 from 259, ... 52: 16 from 65 539 */
    return (1u << (c - 36u)) + 3u;
}

/* the Huffman tree description at p (RFC 8878 4.2.1) into S->huf; -> bytes used, or MZ_ZS_ERR */
MZ_DEV uint32_t mz_zs_huf_read(mz_zs_ctx *C, mz_zs_lds *S, uint32_t p, uint32_t end) {
    MZ_LANE_DECL
    uint32_t hb, n = 0, used, sum = 0, mb, rest, ones = 0;
    if (p >= end) return MZ_ZS_ERR;
    hb = mz_zs_byte(C, S, p);
    MZ_WAVE_SYNC();
    if (hb >= 128u) { /* direct: 4 bits per weight */
        n = hb - 127u;
        used = 1u + ((n + 1u) >> 1);
        if (used > end - p) return MZ_ZS_ERR;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t b = mz_zs_byte(C, S, p + 1u + (i >> 1));
            S->weights[i] = (uint8_t)((i & 1u) ? (b & 15u) : (b >> 4));
        }
        MZ_ZS_STAT(mz_zs_stat.weights_direct++);
    } else { /* FSE-compressed: two interleaved states until the stream is read past its start */
        uint32_t al = 0, nsym = 0, hs, s1, s2;
        mz_zs_bits B;
        if (hb == 0 || hb > end - p - 1u) return MZ_ZS_ERR;
        used = 1u + hb;
        hs = mz_zs_fse_read(C, S, p + 1u, p + used, 6u, 12u, &al, &nsym);
        if (hs == MZ_ZS_ERR) return MZ_ZS_ERR;
        mz_zs_fse_build(S->wt, S, nsym, al);
        if (!mz_zs_bits_open(C, S, &B, p + 1u + hs, hb - hs)) return MZ_ZS_ERR;
        s1 = mz_zs_bits_read(C, S, &B, al);
        s2 = mz_zs_bits_read(C, S, &B, al);
        for (;;) {
            uint32_t e;
            if (n >= 254u) return MZ_ZS_ERR;
            e = MZ_UNIFORM(S->wt[s1]);
            S->weights[n++] = (uint8_t)e;
            s1 = (e >> 16) + mz_zs_bits_read(C, S, &B, (e >> 8) & 255u);
            if (B.bits < 0) {
                S->weights[n++] = (uint8_t)MZ_UNIFORM(S->wt[s2]);
                break;
            }
            if (n >= 254u) return MZ_ZS_ERR;
            e = MZ_UNIFORM(S->wt[s2]);
            S->weights[n++] = (uint8_t)e;
            s2 = (e >> 16) + mz_zs_bits_read(C, S, &B, (e >> 8) & 255u);
            if (B.bits < 0) {
                S->weights[n++] = (uint8_t)MZ_UNIFORM(S->wt[s1]);
                break;
            }
        }
        MZ_ZS_STAT(mz_zs_stat.weights_fse++);
    }
    MZ_WAVE_SYNC();
    /* the last weight is what completes the sum to a power of two */
    for (uint32_t w = 0; w < 16u; w++) S->rank[w] = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t w = MZ_UNIFORM(S->weights[i]);
        if (w > MZ_ZS_HUF_LOG_MAX + 1u) return MZ_ZS_ERR;
        if (w) {
            sum += 1u << (w - 1u);
            S->rank[w] = MZ_UNIFORM(S->rank[w]) + 1u;
        }
    }
    if (sum == 0) return MZ_ZS_ERR;
    mb = mz_zs_highbit(sum) + 1u;
    if (mb > MZ_ZS_HUF_LOG_MAX) return MZ_ZS_ERR;
    rest = (1u << mb) - sum;
    if (rest & (rest - 1u)) return MZ_ZS_ERR;
    {
        const uint32_t lw = mz_zs_highbit(rest) + 1u;
        S->weights[n] = (uint8_t)lw;
        S->rank[lw] = MZ_UNIFORM(S->rank[lw]) + 1u;
        n++;
    }
    ones = MZ_UNIFORM(S->rank[1]);
    if (ones < 2u || (ones & 1u)) return MZ_ZS_ERR; /* (libzstd's HUF_readStats: the two longest codes are siblings) */
    /* rank[w] := the first cell of weight w: the lowest weights (longest codes) take the lowest cells */
    {
        uint32_t start = 0;
        for (uint32_t w = 1; w <= mb; w++) {
            const uint32_t c = MZ_UNIFORM(S->rank[w]);
            S->rank[w] = start;
            start += c << (w - 1u);
        }
    }
    MZ_WAVE_SYNC();
    MZ_LANES { /* a lane per symbol: its place among the symbols of its weight, then its cells */
        for (uint32_t s = (uint32_t)lane; s < n; s += 64u) {
            const uint32_t w = S->weights[s];
            if (w) {
                uint32_t c = 0;
                for (uint32_t j = 0; j < s; j++) c += S->weights[j] == w;
                const uint32_t len = 1u << (w - 1u), first = S->rank[w] + c * len;
                const uint16_t cell = (uint16_t)(s | ((mb + 1u - w) << 8));
                for (uint32_t u = 0; u < len; u++) S->huf[first + u] = cell;
            }
        }
    }
    MZ_WAVE_SYNC();
    C->huf_log = mb;
    C->have_huf = 1;
    return used;
}

/* one Huffman stream of n bytes at p decoded by ONE lane into cnt bytes at dst; -> 0, or 1 if the stream has no marker or
 * is not used up exactly by cnt symbols */
MZ_DEV uint32_t mz_zs_huf_stream(const uint8_t *p, uint32_t n, uint8_t *dst, uint32_t cnt, const uint16_t *tab, uint32_t tl) {
    int32_t bits;
    uint32_t last;
    if (n == 0) return 1;
    last = p[n - 1u];
    if (last == 0) return 1;
    bits = (int32_t)(8u * (n - 1u) + mz_zs_highbit(last));
    for (uint32_t i = 0; i < cnt; i++) {
        const int32_t lo = bits - (int32_t)tl, b = lo >> 3; /* (arithmetic shift: the floor also below 0) */
        uint32_t v = 0, e;
        for (int32_t j = 0; j < 3; j++)
            if (b + j >= 0 && (uint32_t)(b + j) < n) v |= (uint32_t)p[b + j] << (8 * j);
        e = tab[(v >> ((uint32_t)lo & 7u)) & ((1u << tl) - 1u)];
        dst[i] = (uint8_t)e;
        bits -= (int32_t)(e >> 8);
    }
    return bits != 0;
}

/* the literals section at p: the literals to C->lit, their number to *lit_n; -> the section's bytes, MZ_ZS_ERR for a data error */
MZ_DEV uint32_t mz_zs_literals(mz_zs_ctx *C, mz_zs_lds *S, uint32_t p, uint32_t end, uint32_t *lit_n) {
    MZ_LANE_DECL
    const uint32_t b0 = mz_zs_byte(C, S, p), type = b0 & 3u, sf = (b0 >> 2) & 3u;
    uint32_t hdr, regen, comp = 0, streams = 1;
    MZ_ZS_STAT(mz_zs_stat.lit[type * 4u + sf]++);
    if (type < 2u) { /* Raw, RLE */
        hdr = (sf & 1u) ? (sf == 1u ? 2u : 3u) : 1u;
        if (hdr > end - p) return MZ_ZS_ERR;
        regen = (sf & 1u) ? (mz_zs_le(C, S, p, hdr) >> 4) : (b0 >> 3);
        if (regen > C->blk_max) return MZ_ZS_ERR;
        if (type == 0) {
            const uint8_t *src = C->in + p + hdr;
            uint8_t *lit = C->lit;
            if (regen > end - p - hdr) return MZ_ZS_ERR;
            MZ_LANES {
                for (uint32_t k = (uint32_t)lane; k < regen; k += 64u) lit[k] = src[k];
            }
            *lit_n = regen;
            return hdr + regen;
        }
        if (hdr + 1u > end - p) return MZ_ZS_ERR;
        {
            const uint32_t v = mz_zs_byte(C, S, p + hdr);
            uint8_t *lit = C->lit;
            MZ_LANES {
                for (uint32_t k = (uint32_t)lane; k < regen; k += 64u) lit[k] = (uint8_t)v;
            }
        }
        *lit_n = regen;
        return hdr + 1u;
    }
    /* Compressed, Treeless */
    hdr = sf < 2u ? 3u : sf + 2u;
    if (hdr > end - p) return MZ_ZS_ERR;
    if (sf < 2u) {
        const uint32_t v = mz_zs_le(C, S, p, 3) >> 4;
        regen = v & 1023u;
        comp = v >> 10;
        streams = sf ? 4u : 1u;
    } else if (sf == 2u) {
        const uint32_t v = mz_zs_le(C, S, p, 4) >> 4;
        regen = v & 16383u;
        comp = v >> 14;
        streams = 4;
    } else {
        const uint32_t v = mz_zs_le(C, S, p, 4) >> 4; /* 28 of the 36 bits */
        regen = v & 262143u;
        comp = (v >> 18) | (mz_zs_byte(C, S, p + 4u) << 10);
        streams = 4;
    }
    if (regen == 0 || regen > C->blk_max || comp > end - p - hdr) return MZ_ZS_ERR;
    {
        uint32_t q = p + hdr, left = comp;
        if (type == 2u) {
            const uint32_t used = mz_zs_huf_read(C, S, q, q + comp);
            if (used == MZ_ZS_ERR) return MZ_ZS_ERR;
            q += used;
            left -= used;
        } else {
            if (!C->have_huf) return MZ_ZS_ERR;
            MZ_ZS_STAT(mz_zs_stat.treeless++);
        }
        MZ_ZSPROF_MARK(C, 0);
        {
            const uint32_t seg = (regen + 3u) >> 2, tl = C->huf_log;
            uint32_t s1 = 0, s2 = 0, s3 = 0;
            uint64_t any;
            PV(uint32_t, bad);
            if (streams == 4u) {
                if (left < 10u) return MZ_ZS_ERR;
                s1 = mz_zs_le(C, S, q, 2);
                s2 = mz_zs_le(C, S, q + 2u, 2);
                s3 = mz_zs_le(C, S, q + 4u, 2);
                q += 6u;
                left -= 6u;
                if (s1 + s2 + s3 > left || 3u * seg > regen) return MZ_ZS_ERR;
                MZ_ZS_STAT(mz_zs_stat.streams4++);
            } else {
                MZ_ZS_STAT(mz_zs_stat.streams1++);
            }
            {
                const uint8_t *src = C->in + q;
                uint8_t *lit = C->lit;
                const uint16_t *tab = S->huf;
                MZ_LANES {
                    P(bad) = 0;
                    if ((uint32_t)lane < streams) {
                        uint32_t so = 0, sn = left, d0 = 0, dn = regen;
                        if (streams == 4u) {
                            so = lane == 0 ? 0u : lane == 1 ? s1 : lane == 2 ? s1 + s2 : s1 + s2 + s3;
                            sn = lane == 0 ? s1 : lane == 1 ? s2 : lane == 2 ? s3 : left - s1 - s2 - s3;
                            d0 = (uint32_t)lane * seg;
                            dn = lane == 3 ? regen - 3u * seg : seg;
                        }
                        P(bad) = mz_zs_huf_stream(src + so, sn, lit + d0, dn, tab, tl);
                    }
                }
            }
            MZ_BALLOT(any, P(bad) != 0u);
            if (any) return MZ_ZS_ERR;
        }
        MZ_ZSPROF_MARK(C, 1);
    }
    *lit_n = regen;
    return hdr + comp;
}

/* one of the three sequence tables according to its mode; -> bytes used, or MZ_ZS_ERR */
MZ_DEV uint32_t mz_zs_seq_table(mz_zs_ctx *C, mz_zs_lds *S, uint32_t which, uint32_t mode, uint32_t p, uint32_t end, uint32_t *al) {
    uint32_t *const tab = which == 0 ? S->ll : which == 1 ? S->of : S->ml;
    const uint32_t max_sym = which == 0 ? 35u : which == 1 ? 31u : 52u, max_al = which == 1 ? 8u : 9u;
    MZ_ZS_STAT(mz_zs_stat.mode[which][mode]++);
    if (mode == 0) {
        const uint32_t n = which == 0 ? 36u : which == 1 ? 29u : 53u;
        MZ_WAVE_SYNC();
        for (uint32_t s = 0; s < n; s++) S->norm[s] = which == 0 ? mz_zs_dll[s] : which == 1 ? mz_zs_dof[s] : mz_zs_dml[s];
        *al = which == 1 ? 5u : 6u;
        mz_zs_fse_build(tab, S, n, *al);
        return 0;
    }
    if (mode == 1) {
        uint32_t sym;
        if (p >= end) return MZ_ZS_ERR;
        sym = mz_zs_byte(C, S, p);
        if (sym > max_sym) return MZ_ZS_ERR;
        mz_zs_fse_rle(tab, sym);
        *al = 0;
        return 1;
    }
    if (mode == 2) {
        uint32_t nsym = 0;
        const uint32_t used = mz_zs_fse_read(C, S, p, end, max_al, max_sym, al, &nsym);
        if (used == MZ_ZS_ERR) return MZ_ZS_ERR;
        mz_zs_fse_build(tab, S, nsym, *al);
        return used;
    }
    return C->have_seq ? 0u : MZ_ZS_ERR; /* repeat: the table and its accuracy log stand */
}

/* a Compressed block [p, end) -> status; C->o moves over what was written */
MZ_DEV int32_t mz_zs_block(mz_zs_ctx *C, mz_zs_lds *S, uint32_t p, uint32_t end) {
    MZ_LANE_DECL
    const uint32_t bo = C->o;
    uint32_t lit_n = 0, lp = 0, nseq, used, b0;
    used = mz_zs_literals(C, S, p, end, &lit_n);
    if (used == MZ_ZS_ERR) return MZHIP_DATA_ERROR;
    p += used;
    MZ_CHASE_FENCE(); /* literals are stored through some lanes' addresses and read through others' */
    MZ_WAVE_SYNC();

    /* ---- the sequences section: count, modes, tables */
    if (p >= end) return MZHIP_DATA_ERROR;
    b0 = mz_zs_byte(C, S, p);
    if (b0 < 128u) {
        nseq = b0;
        p += 1u;
    } else if (b0 < 255u) {
        if (end - p < 2u) return MZHIP_DATA_ERROR;
        nseq = ((b0 - 128u) << 8) + mz_zs_byte(C, S, p + 1u);
        p += 2u;
    } else {
        if (end - p < 3u) return MZHIP_DATA_ERROR;
        nseq = mz_zs_le(C, S, p + 1u, 2) + 0x7F00u;
        p += 3u;
    }
    if (nseq == 0) {
        if (p != end) return MZHIP_DATA_ERROR;
    } else {
        uint32_t modes, sll, sof, sml;
        mz_zs_bits B;
        if (p >= end) return MZHIP_DATA_ERROR;
        modes = mz_zs_byte(C, S, p);
        p += 1u;
        if (modes & 3u) return MZHIP_DATA_ERROR;
        used = mz_zs_seq_table(C, S, 0, modes >> 6, p, end, &C->al_ll);
        if (used == MZ_ZS_ERR) return MZHIP_DATA_ERROR;
        p += used;
        used = mz_zs_seq_table(C, S, 1, (modes >> 4) & 3u, p, end, &C->al_of);
        if (used == MZ_ZS_ERR) return MZHIP_DATA_ERROR;
        p += used;
        used = mz_zs_seq_table(C, S, 2, (modes >> 2) & 3u, p, end, &C->al_ml);
        if (used == MZ_ZS_ERR) return MZHIP_DATA_ERROR;
        p += used;
        C->have_seq = 1;
        if (!mz_zs_bits_open(C, S, &B, p, end - p)) return MZHIP_DATA_ERROR;
        sll = mz_zs_bits_read(C, S, &B, C->al_ll);
        sof = mz_zs_bits_read(C, S, &B, C->al_of);
        sml = mz_zs_bits_read(C, S, &B, C->al_ml);
        if (B.bits < 0) return MZHIP_DATA_ERROR;
        MZ_ZSPROF_MARK(C, 0);

        for (uint32_t i = 0; i < nseq; i++) {
            const uint32_t ell = MZ_UNIFORM(S->ll[sll]), eof = MZ_UNIFORM(S->of[sof]), eml = MZ_UNIFORM(S->ml[sml]);
            const uint32_t ofc = eof & 255u;
            uint32_t nb_ll, nb_ml, ll, ml, ofv, dist;
            ofv = (1u << ofc) + mz_zs_bits_read(C, S, &B, ofc); /* offset codes 0 .. 31 */
            ml = mz_zs_ml_base(eml & 255u, &nb_ml);
            ml += mz_zs_bits_read(C, S, &B, nb_ml);
            ll = mz_zs_ll_base(ell & 255u, &nb_ll);
            ll += mz_zs_bits_read(C, S, &B, nb_ll);
            MZ_ZS_STAT(mz_zs_stat.ll_code[ell & 255u]++);
            MZ_ZS_STAT(mz_zs_stat.ml_code[eml & 255u]++);
            MZ_ZS_STAT(mz_zs_stat.of_code[ofc]++);
            if (i + 1u < nseq) { /* the last sequence leaves the states alone */
                sll = (ell >> 16) + mz_zs_bits_read(C, S, &B, (ell >> 8) & 255u);
                sml = (eml >> 16) + mz_zs_bits_read(C, S, &B, (eml >> 8) & 255u);
                sof = (eof >> 16) + mz_zs_bits_read(C, S, &B, (eof >> 8) & 255u);
            }
            if (B.bits < 0) return MZHIP_DATA_ERROR;
            /* ---- repeat offsets */
            if (ofv > 3u) {
                dist = ofv - 3u;
                C->rep2 = C->rep1;
                C->rep1 = C->rep0;
                C->rep0 = dist;
                MZ_ZS_STAT(mz_zs_stat.rep_rule[0]++);
            } else {
                const uint32_t idx = ofv - 1u + (ll == 0u);
                MZ_ZS_STAT(mz_zs_stat.rep_rule[ofv + (ll == 0u ? 3u : 0u)]++);
                if (idx == 0) {
                    dist = C->rep0;
                } else {
                    dist = idx == 1u ? C->rep1 : idx == 2u ? C->rep2 : C->rep0 - 1u;
                    if (dist == 0) return MZHIP_DATA_ERROR;
                    if (idx != 1u) C->rep2 = C->rep1;
                    C->rep1 = C->rep0;
                    C->rep0 = dist;
                }
            }
            MZ_ZSPROF_MARK(C, 2);
            /* ---- execution: literals and match in one pass of the lanes */
            {
                const uint32_t o = C->o, m0 = o + ll;
                if (ll + ml > C->out_cap - o) return MZHIP_OUT_FULL;
                if (ll > lit_n - lp) return MZHIP_DATA_ERROR;
                if (dist > m0 - C->fo) return MZHIP_DATA_ERROR;
                if (m0 + ml - bo > C->blk_max) return MZHIP_DATA_ERROR;
                if (dist < ml) MZ_ZS_STAT(mz_zs_stat.overlap[dist <= 70u ? dist : 71u]++);
                MZ_CHASE_FENCE(); /* behind the stores of the sequences before this one */
                MZ_WAVE_SYNC();
                {
                    uint8_t *out = C->out;
                    const uint8_t *lit = C->lit + lp;
                    MZ_LANES {
                        for (uint32_t k = (uint32_t)lane; k < ll; k += 64u) out[o + k] = lit[k];
                        for (uint32_t k = (uint32_t)lane; k < ml; k += 64u) {
                            const uint32_t src = m0 - dist + (dist < ml ? k % dist : k);
                            out[m0 + k] = src >= o ? lit[src - o] : out[src];
                        }
                    }
                }
                lp += ll;
                C->o = m0 + ml;
            }
            MZ_ZSPROF_MARK(C, 3);
        }
        if (B.bits != 0) return MZHIP_DATA_ERROR;
    }
    /* ---- the literals behind the last sequence */
    {
        const uint32_t n = lit_n - lp, o = C->o;
        uint8_t *out = C->out;
        const uint8_t *lit = C->lit + lp;
        if (n > C->out_cap - o) return MZHIP_OUT_FULL;
        if (o + n - bo > C->blk_max) return MZHIP_DATA_ERROR;
        MZ_LANES {
            for (uint32_t k = (uint32_t)lane; k < n; k += 64u) out[o + k] = lit[k];
        }
        C->o = o + n;
    }
    MZ_ZSPROF_MARK(C, 3);
    return MZHIP_OK;
}

#define MZ_XXH_P1 0x9E3779B185EBCA87ull
#define MZ_XXH_P2 0xC2B2AE3D27D4EB4Full
#define MZ_XXH_P3 0x165667B19E3779F9ull
#define MZ_XXH_P4 0x85EBCA77C2B2AE63ull
#define MZ_XXH_P5 0x27D4EB2F165667C5ull
MZ_DEV uint64_t mz_xxh_rotl(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
MZ_DEV uint64_t mz_xxh_round(uint64_t acc, uint64_t v) { return mz_xxh_rotl(acc + v * MZ_XXH_P2, 31) * MZ_XXH_P1; }
MZ_DEV uint64_t mz_xxh_merge(uint64_t h, uint64_t v) { return (h ^ mz_xxh_round(0, v)) * MZ_XXH_P1 + MZ_XXH_P4; }

/* the low 32 bits of XXH64(d[0 .. n), seed 0): the four accumulators on lanes 0 .. 3, 8 bytes of every 32 each */
MZ_DEV uint32_t mz_zs_xxh64(const uint8_t *d, uint32_t n) {
    MZ_LANE_DECL
    uint64_t h = MZ_XXH_P5;
    uint32_t i = 0;
    if (n >= 32u) {
        const uint32_t stripes = n >> 5;
        PV(uint32_t, lo);
        PV(uint32_t, hi);
        MZ_LANES {
            const uint32_t k = (uint32_t)lane & 3u;
            uint64_t v = k == 0 ? MZ_XXH_P1 + MZ_XXH_P2 : k == 1u ? MZ_XXH_P2 : k == 2u ? 0ull : 0ull - MZ_XXH_P1;
            if ((uint32_t)lane < 4u)
                for (uint32_t s = 0; s < stripes; s++) v = mz_xxh_round(v, mz_ld8(d + 32u * (size_t)s + 8u * k));
            P(lo) = (uint32_t)v;
            P(hi) = (uint32_t)(v >> 32);
        }
        {
            const uint64_t v1 = ((uint64_t)MZ_READLANE(hi, 0) << 32) | MZ_READLANE(lo, 0), v2 = ((uint64_t)MZ_READLANE(hi, 1) << 32) | MZ_READLANE(lo, 1);
            const uint64_t v3 = ((uint64_t)MZ_READLANE(hi, 2) << 32) | MZ_READLANE(lo, 2), v4 = ((uint64_t)MZ_READLANE(hi, 3) << 32) | MZ_READLANE(lo, 3);
            h = mz_xxh_rotl(v1, 1) + mz_xxh_rotl(v2, 7) + mz_xxh_rotl(v3, 12) + mz_xxh_rotl(v4, 18);
            h = mz_xxh_merge(h, v1);
            h = mz_xxh_merge(h, v2);
            h = mz_xxh_merge(h, v3);
            h = mz_xxh_merge(h, v4);
        }
        i = stripes << 5;
    }
    h += n;
    for (; i + 8u <= n; i += 8u) {
        const uint64_t k1 = ((uint64_t)MZ_UNIFORM(mz_ld4(d + i + 4u)) << 32) | MZ_UNIFORM(mz_ld4(d + i));
        h = mz_xxh_rotl(h ^ mz_xxh_round(0, k1), 27) * MZ_XXH_P1 + MZ_XXH_P4;
    }
    if (i + 4u <= n) {
        h = mz_xxh_rotl(h ^ ((uint64_t)MZ_UNIFORM(mz_ld4(d + i)) * MZ_XXH_P1), 23) * MZ_XXH_P2 + MZ_XXH_P3;
        i += 4u;
    }
    for (; i < n; i++) h = mz_xxh_rotl(h ^ ((uint64_t)MZ_UNIFORM(d[i]) * MZ_XXH_P5), 11) * MZ_XXH_P1;
    h ^= h >> 33;
    h *= MZ_XXH_P2;
    h ^= h >> 29;
    h *= MZ_XXH_P3;
    h ^= h >> 32;
    return (uint32_t)h;
}

#define MZ_ZS_FAIL(code)  \
    do {                  \
        st = (code);      \
        goto done;        \
    } while (0)

MZ_DEV void mz_zstd_entry(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, mz_zs_lds *S, const uint32_t *crc_tab,
                          const mzhip_crc_tables *tabs, uint8_t *scratch, mz_zs_result *res) {
    MZ_LANE_DECL
    mz_zs_ctx ctx;
    mz_zs_ctx *const C = &ctx;
    int32_t st = MZHIP_OK;
    uint32_t p = 0, o_good = 0, crc = 0, magic = 0, fhd = 0, single = 0, n = 0, have_fcs = 0, last = 0, bh = 0, type = 0, bs = 0, wd = 0;
    uint64_t wsize = 0, fcs = 0;
    C->in = in;
    C->in_len = in_len;
    C->base = 0u - MZ_ZS_INBUF;
    C->out = out;
    C->out_cap = out_cap;
    C->lit = scratch;
    C->o = 0;
    C->fo = 0;
    C->blk_max = 0;
    C->rep0 = C->rep1 = C->rep2 = 0;
    C->have_huf = C->huf_log = C->have_seq = 0;
    C->al_ll = C->al_of = C->al_ml = 0;
    MZ_ZSPROF_INIT(C);

    if (in_len == 0) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
    while (p < in_len) {
        /* ---- frame header */
        if (in_len - p < 4u) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
        magic = mz_zs_le(C, S, p, 4);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) { /* a skippable frame: its size, then that many bytes */
            if (in_len - p < 8u) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
            n = mz_zs_le(C, S, p + 4u, 4);
            if (n > in_len - p - 8u) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
            p += 8u + n;
            MZ_ZS_STAT(mz_zs_stat.skippable++);
            continue;
        }
        if (magic != 0xFD2FB528u) MZ_ZS_FAIL(MZHIP_DATA_ERROR);
        p += 4u;
        if (p >= in_len) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
        fhd = mz_zs_byte(C, S, p);
        p += 1u;
        if (fhd & 8u) MZ_ZS_FAIL(MZHIP_DATA_ERROR);
        single = (fhd >> 5) & 1u;
        if (!single) {
            if (p >= in_len) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
            wd = mz_zs_byte(C, S, p);
            p += 1u;
            if (10u + (wd >> 3) > 31u) MZ_ZS_FAIL(MZHIP_DATA_ERROR); /* libzstd's ZSTD_WINDOWLOG_MAX */
            wsize = 1ull << (10u + (wd >> 3));
            wsize += (wsize >> 3) * (wd & 7u);
        }
        n = (fhd & 3u) == 3u ? 4u : (fhd & 3u); /* Dictionary_ID */
        if (n > in_len - p) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
        if (mz_zs_le(C, S, p, n) != 0) MZ_ZS_FAIL(MZHIP_UNSUPPORTED);
        p += n;
        n = (fhd >> 6) ? (1u << (fhd >> 6)) : single; /* Frame_Content_Size */
        if (n > in_len - p) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
        have_fcs = n != 0;
        fcs = mz_zs_le(C, S, p, n < 4u ? n : 4u);
        if (n == 8u) fcs |= (uint64_t)mz_zs_le(C, S, p + 4u, 4) << 32;
        if (n == 2u) fcs += 256u;
        p += n;
        if (single) wsize = fcs;
        C->blk_max = wsize < MZ_ZS_BLOCK_MAX ? (uint32_t)wsize : MZ_ZS_BLOCK_MAX;
        C->rep0 = 1;
        C->rep1 = 4;
        C->rep2 = 8;
        C->have_huf = 0;
        C->have_seq = 0;
        C->fo = C->o;
        MZ_ZS_STAT(mz_zs_stat.frames++);

        /* ---- blocks */
        do {
            if (in_len - p < 3u) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
            bh = mz_zs_le(C, S, p, 3);
            p += 3u;
            last = bh & 1u;
            type = (bh >> 1) & 3u;
            bs = bh >> 3;
            if (type == 3u) MZ_ZS_FAIL(MZHIP_DATA_ERROR);
            if (bs > C->blk_max) MZ_ZS_FAIL(MZHIP_DATA_ERROR);
            if (type == 0) {
                if (bs > in_len - p) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
                if (bs > out_cap - C->o) MZ_ZS_FAIL(MZHIP_OUT_FULL);
                MZ_LANES {
                    for (uint32_t k = (uint32_t)lane; k < bs; k += 64u) out[C->o + k] = in[p + k];
                }
                p += bs;
                C->o += bs;
            } else if (type == 1u) {
                if (p >= in_len) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
                if (bs > out_cap - C->o) MZ_ZS_FAIL(MZHIP_OUT_FULL);
                n = mz_zs_byte(C, S, p);
                MZ_LANES {
                    for (uint32_t k = (uint32_t)lane; k < bs; k += 64u) out[C->o + k] = (uint8_t)n;
                }
                p += 1u;
                C->o += bs;
            } else {
                if (bs > in_len - p) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
                if (bs < 3u) MZ_ZS_FAIL(MZHIP_DATA_ERROR); /* (libzstd's MIN_CBLOCK_SIZE) */
                if (bs >= MZ_ZS_BLOCK_MAX) MZ_ZS_FAIL(MZHIP_DATA_ERROR); /* a Compressed block is smaller than what it holds */
                st = mz_zs_block(C, S, p, p + bs);
                if (st != MZHIP_OK) {
                    p -= 3u;
                    goto done;
                }
                p += bs;
            }
            o_good = C->o;
        } while (!last);

        if (have_fcs && (uint64_t)(C->o - C->fo) != fcs) MZ_ZS_FAIL(MZHIP_DATA_ERROR);
        if (fhd & 4u) { /* Content_Checksum */
            if (in_len - p < 4u) MZ_ZS_FAIL(MZHIP_BUF_ERROR);
            n = mz_zs_le(C, S, p, 4);
            MZ_CHASE_FENCE();
            MZ_WAVE_SYNC();
            MZ_ZSPROF_MARK(C, 0);
            if (mz_zs_xxh64(out + C->fo, C->o - C->fo) != n) MZ_ZS_FAIL(MZHIP_DATA_ERROR);
            MZ_ZSPROF_MARK(C, 4);
            p += 4u;
            MZ_ZS_STAT(mz_zs_stat.checksums++);
        }
    }

done:
    /* the ZIP CRC-32 of what stands: the K2 fold over the finished bytes */
    MZ_CHASE_FENCE();
    MZ_WAVE_SYNC();
    MZ_ZSPROF_MARK(C, 0);
    {
        PV(uint32_t, acc);
        PV(uint32_t, tmp);
        uint32_t folded = 0;
        MZ_LANES { P(acc) = (lane == 0) ? 0xFFFFFFFFu : 0u; }
        MZ_CRC_FOLD_TILES(acc, folded, out, o_good, crc_tab, tabs->kx);
        MZ_CRC_FINISH(crc, acc, tmp, folded, out, o_good, crc_tab, tabs);
    }
    MZ_ZSPROF_MARK(C, 4);
    MZ_ZSPROF_FLUSH(C)
    res->out_len = o_good;
    res->in_used = p;
    res->crc = crc;
    res->status = st;
}

#endif
