/* bzip2_enc_core.h -- one bzip2 stream (ZIP method 12, the reference's mz_strm_bzip.c over BZ2_bzCompress) written by one wave.
 *
 * Written in the wave.h vocabulary: the same text is the gfx950 kernel body (k_bzip2_encode_batch) and, under
 * g++ -DMZHIP_HOST_EMUL, the host build the CPU tests run (tests/emul/emul_bzip2_enc.cpp).  The stream is "BZh" + digit, the
 * blocks one after the other (they join at bit granularity: one bit writer runs through the whole stream), the end magic
 * and the combined CRC, padded to a byte.  Per block a wave
 *   1. takes input, 64 bytes per step, through the first run-length stage: run boundaries by comparing neighbours, the place
 *      in the run by a ballot, the symbols' places by a wave scan.  The block closes in front of the first byte with which
 *      its symbols -- the count that closes the open run included -- would exceed 100000 * level - 19 (libbz2's nblockMAX);
 *      a run lying across the cut is closed there and starts again in the next block.  The block CRC (MSB-first,
 *      0x04C11DB7) of the bytes taken: 64 strips, a lane each, joined by multiplying with x^(8 * strip) mod P;
 *   2. sorts the n cyclic rotations: a stable counting sort by the first byte, then prefix doubling as Manber and Myers do
 *      it.  Round h walks the rotations in their order so far, 64 per step: rotation j puts rotation j - h into the next free
 *      slot of ITS group (same first h bytes), so every group ends up ordered by the h bytes behind.  The scatter is the
 *      shape of the decoder's stage 4 with rank keys: the same-key mask of the lanes by one ballot per key bit,
 *      MZ_RANK_BELOW, the group's fill count moved on by the key's last lane.  A second pass re-ranks: a boundary wherever
 *      the old group or the rank h further on changes, the rank = the place of the latest boundary (ballot + clz).  It stops
 *      when every rank is unique or h >= n: at most ceil(log2 n) rounds of 3 * n / 64 steps for EVERY input, no fallback,
 *      and a periodic block (equal rotations, ranks never unique) ends with h >= n; origPtr is where rotation 0 landed;
 *   3. move-to-front over the last column with the list in LDS (found by the lanes, four entries each; shifted by the
 *      lanes), zero runs as RUNA / RUNB, then EOB: 16-bit symbols to the scratch;
 *   4. chooses 2 .. 6 tables by libbz2's thresholds, starts from its frequency partition and refines MZ_BZE_ITERS times:
 *      every group of 50 symbols is priced against every table, a lane per group, then each table is refitted to its groups
 *      (Huffman by two queues over the sorted frequencies, halved until no code is longer than 17).  A table that costs its
 *      groups more than the flat code of the alphabet is replaced by the flat code;
 *   5. writes header, symbol map, selectors (move-to-front, unary), the delta-coded lengths -- wave-uniform, through a 64-bit
 *      accumulator -- and the symbols, 64 per step: a scan of the code lengths gives every lane its bit offset, the codes
 *      are OR-ed into the LDS window.  The window is flushed to the output in whole 32-bit words by the lanes; nothing is
 *      stored outside [out, out + out_cap), and an output that does not fit ends the entry with MZHIP_OUT_FULL, out_len 0;
 *   6. after the stream folds the ZIP CRC-32 over the INPUT with the K2 tiles.
 *
 * LDS: sizeof(mz_bze_lds) = 27 408 bytes (26.8 KiB) per wave.  Scratch in HBM per wave, for a capacity of C symbols (MZ_BZE_CAP_SYMS: the
 * smaller of 100000 * level and the RLE1 bound of the largest entry, rounded up to 64): MZ_BZE_SCRATCH_BYTES(C) = 17 C +
 * 18 048 -- two rotation orders and two rank arrays of 4 C each (the second rank array is the scatter's fill counts, the
 * first holds the 16-bit symbols once the sort is done), C symbols of the block, 18 002 selectors.
 */
#ifndef MZHIP_BZIP2_ENC_CORE_H
#define MZHIP_BZIP2_ENC_CORE_H

#include "crc32_core.h"
#include "wave.h"

#define MZ_BZE_MAX_SELECTORS 18002u
#define MZ_BZE_GROUPS 6u
#define MZ_BZE_ALPHA 258u
#define MZ_BZE_MAXLEN 17u /* libbz2's own limit; the format's is 20 */
#define MZ_BZE_ITERS 4u
#define MZ_BZE_G 50u
#define MZ_BZE_WIN 256u /* words of the bit window */
#define MZ_BZE_SEL_BYTES 18048u
/* symbols a wave's scratch holds: min(100000 * level, in_len + in_len / 4 + 1), rounded up to 64 */
#define MZ_BZE_RLE_BOUND(n) ((uint64_t)(n) + (uint64_t)(n) / 4u)
#define MZ_BZE_CAP_SYMS(max_in_len, level)                                                                                        \
    ((uint32_t)((((MZ_BZE_RLE_BOUND(max_in_len) + 1u < 100000ull * (uint64_t)(level)) ? MZ_BZE_RLE_BOUND(max_in_len) + 1u       \
                                                                                         : 100000ull * (uint64_t)(level)) + 63u) & ~63ull))
#define MZ_BZE_SCRATCH_BYTES(c) ((((uint64_t)(c) * 17u + MZ_BZE_SEL_BYTES) + 255u) & ~(uint64_t)255u)

/* the block-size digit of a level as mz_stream_bzip_set_prop_int64 maps it: 1 .. 9, -1 = 6; 0 = not a level */
#define MZ_BZE_LEVEL(level) ((level) == -1 ? 6u : ((level) >= 1 && (level) <= 9) ? (uint32_t)(level) : 0u)
/* An output size that always suffices (include/mzhip.h derives it): R = in_len + in_len / 4 symbols behind the first
 * run-length stage in nb <= R / (100000 * level - 24) + 1 blocks; per block n + 2 symbols at most, 9 bits each at most, a
 * selector of at most 6 bits per 50 symbols begun, 51 509 bits of header and tables; 14 bytes of frame. */
#define MZ_BZE_BOUND(in_len, digit)                                                                                          \
    (14u + ((9u * (MZ_BZE_RLE_BOUND(in_len) + 2u * (MZ_BZE_RLE_BOUND(in_len) / (100000ull * (digit) - 24u) + 1u)) +           \
             6u * ((MZ_BZE_RLE_BOUND(in_len) + 2u * (MZ_BZE_RLE_BOUND(in_len) / (100000ull * (digit) - 24u) + 1u)) / 50u +    \
                   (MZ_BZE_RLE_BOUND(in_len) / (100000ull * (digit) - 24u) + 1u)) +                                           \
             51509u * (MZ_BZE_RLE_BOUND(in_len) / (100000ull * (digit) - 24u) + 1u) + 7u) / 8u))

typedef struct mz_bze_lds {
    uint64_t lenpack[MZ_BZE_ALPHA + 2u]; /* the tables' lengths of a symbol, 10 bits each: 50 symbols sum without a carry */
    uint32_t win[MZ_BZE_WIN];
    uint32_t bzcrc[256];
    uint32_t hist[256];   /* byte counts of the block's symbols */
    uint32_t start0[256]; /* where a byte value's rotations start */
    uint32_t start[256];  /* ... moved on by the scatter */
    uint32_t mfreq[MZ_BZE_ALPHA + 2u];
    uint32_t rfreq[MZ_BZE_GROUPS][MZ_BZE_ALPHA + 2u];
    uint32_t code[MZ_BZE_GROUPS][MZ_BZE_ALPHA + 2u];
    uint32_t hf[MZ_BZE_ALPHA + 2u];  /* Huffman: the frequencies as they are halved, */
    uint32_t hw[MZ_BZE_ALPHA + 2u];  /* ... sorted (the leaves), */
    uint32_t hiw[MZ_BZE_ALPHA + 2u]; /* the inner nodes' weights in the order they are made */
    uint32_t lcount[24], fcode[24];
    uint16_t hparent[2u * MZ_BZE_ALPHA + 4u];
    uint16_t horder[MZ_BZE_ALPHA + 2u];
    uint8_t len[MZ_BZE_GROUPS][MZ_BZE_ALPHA + 2u];
    uint8_t mtf[256];
} mz_bze_lds;

typedef struct mz_bze_result {
    uint32_t out_len; /* 0 unless the status is 0 */
    uint32_t crc;     /* CRC-32 of the input */
    int32_t status;
} mz_bze_result;

/* MSB-first bit writer: pending bits in acc (cnt < 32 of them), whole words in the window win[0 .. wn); every word from wn
 * on is zero, except while the lanes code symbols (then win[wn] holds the pending bits, top-aligned) */
typedef struct mz_bze_bits {
    uint8_t *out;
    uint32_t out_cap, o, wn, cnt, fail;
    uint64_t acc;
} mz_bze_bits;

/* the window's whole words to the output, the word behind them (pending bits or zero) to the front */
MZ_DEV void mz_bze_flush(mz_bze_bits *W, mz_bze_lds *S) {
    MZ_LANE_DECL
    const uint32_t wn = W->wn, need = 4u * wn;
    uint32_t part;
    MZ_WAVE_SYNC();
    if (need > W->out_cap - W->o) W->fail = 1u;
    if (!W->fail) {
        MZ_LANES {
            for (uint32_t w = (uint32_t)lane; w < wn; w += 64u) mz_st4(W->out + W->o + 4u * w, __builtin_bswap32(S->win[w]));
        }
        W->o += need;
    }
    part = MZ_UNIFORM(S->win[wn]);
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < MZ_BZE_WIN / 64u; k++) S->win[(uint32_t)lane + 64u * k] = 0u;
    }
    MZ_WAVE_SYNC();
    S->win[0] = part; /* wave-uniform: stored by all lanes */
    MZ_WAVE_SYNC();
    W->wn = 0;
}

/* n <= 32 bits, v < 2^n */
MZ_DEV void mz_bze_put(mz_bze_bits *W, mz_bze_lds *S, uint32_t n, uint32_t v) {
    W->acc = (W->acc << n) | (uint64_t)v;
    W->cnt += n;
    if (W->cnt >= 32u) {
        W->cnt -= 32u;
        S->win[W->wn] = (uint32_t)(W->acc >> W->cnt);
        W->wn++;
        W->acc &= (1ull << W->cnt) - 1ull;
        if (W->wn + 2u >= MZ_BZE_WIN) mz_bze_flush(W, S);
    }
}

/* a * b mod P over GF(2), bit i = x^i (the MSB-first CRC register as a polynomial) */
MZ_DEV uint32_t mz_bze_gfmul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 31; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x80000000u) ? 0x04C11DB7u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

/* A complete set of code lengths 1 .. MZ_BZE_MAXLEN for freq[0 .. alpha) (zero counts as one) into len[]: the symbols sorted by
 * (frequency, index) with a lane per symbol, Huffman's tree by two queues (wave-uniform), depths by walking up, a lane per
 * leaf; while a code is too long the frequencies are halved (1 + f / 2, as libbz2 does) and the tree is made again. */
MZ_DEV void mz_bze_make_lengths(mz_bze_lds *S, const uint32_t *freq, uint8_t *len, uint32_t alpha) {
    MZ_LANE_DECL
    const uint32_t root = 2u * alpha - 2u;
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t i = (uint32_t)lane; i < alpha; i += 64u) S->hf[i] = freq[i] ? freq[i] : 1u;
    }
    for (uint32_t tries = 0;; tries++) {
        uint32_t a = 0, b = 0, m = 0;
        uint64_t too_long = 0;
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t i = (uint32_t)lane; i < alpha; i += 64u) {
                const uint32_t f = S->hf[i];
                uint32_t r = 0;
                for (uint32_t j = 0; j < alpha; j++) {
                    const uint32_t g = S->hf[j];
                    r += (g < f) || (g == f && j < i);
                }
                S->hw[r] = f;
                S->horder[r] = (uint16_t)i;
            }
        }
        MZ_WAVE_SYNC();
        for (m = 0; m + 1u < alpha; m++) { /* the two lightest nodes; a leaf before an inner node of the same weight */
            uint32_t w = 0;
            for (int k = 0; k < 2; k++) {
                const uint32_t lw = a < alpha ? MZ_UNIFORM(S->hw[a < alpha ? a : 0u]) : 0xFFFFFFFFu;
                const uint32_t iw = b < m ? MZ_UNIFORM(S->hiw[b < m ? b : 0u]) : 0xFFFFFFFFu;
                if (a < alpha && (b >= m || lw <= iw)) {
                    S->hparent[a] = (uint16_t)(alpha + m);
                    w += lw;
                    a++;
                } else {
                    S->hparent[alpha + b] = (uint16_t)(alpha + m);
                    w += iw;
                    b++;
                }
            }
            S->hiw[m] = w;
        }
        MZ_WAVE_SYNC();
        {
            PV(uint32_t, deep);
            MZ_LANES {
                P(deep) = 0;
                for (uint32_t r = (uint32_t)lane; r < alpha; r += 64u) {
                    uint32_t d = 0, p = r;
                    while (p != root) {
                        p = S->hparent[p];
                        d++;
                    }
                    if (d > MZ_BZE_MAXLEN) P(deep) = 1;
                    len[S->horder[r]] = (uint8_t)d;
                }
            }
            MZ_BALLOT(too_long, P(deep));
        }
        if (!too_long) break; /* (frequencies of 1 and 2 alone give no code longer than 10: 21 halvings at the most) */
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t i = (uint32_t)lane; i < alpha; i += 64u) S->hf[i] = 1u + S->hf[i] / 2u;
        }
    }
    MZ_WAVE_SYNC();
}

/* the flat code of `alpha` symbols: 2^L - alpha symbols of L - 1 bits in front, the rest L = ceil(log2 alpha) bits */
MZ_DEV uint32_t mz_bze_flat_len(uint32_t i, uint32_t alpha) {
    uint32_t L = 1;
    while ((1u << L) < alpha) L++;
    return i < (1u << L) - alpha ? L - 1u : L;
}

#define MZ_BZE_PUT(n, v) mz_bze_put(&W, S, (uint32_t)(n), (uint32_t)(v))

/* level 1 .. 9; cap_syms: the symbols the scratch holds (MZ_BZE_CAP_SYMS of the launch); scratch: MZ_BZE_SCRATCH_BYTES(cap_syms).
 * An entry longer than the launch was sized for is still written correctly, in blocks the scratch holds. */
MZ_DEV void mz_bzip2_enc_entry(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t level, uint32_t cap_syms,
                               mz_bze_lds *S, const uint32_t *crc_tab, const mzhip_crc_tables *tabs, uint8_t *scratch, mz_bze_result *res) {
    MZ_LANE_DECL
    uint32_t *const A0 = (uint32_t *)scratch;
    uint32_t *const A1 = A0 + cap_syms;
    uint32_t *const R0 = A1 + cap_syms;
    uint32_t *const R1 = R0 + cap_syms;
    uint8_t *const blk = (uint8_t *)(R1 + cap_syms);
    uint8_t *const sel = blk + cap_syms;
    uint16_t *const mtfv = (uint16_t *)R0; /* the rank arrays are dead when the symbols are made */
    const uint32_t bmax = (100000u * level - 19u < cap_syms - 1u) ? 100000u * level - 19u : cap_syms - 1u;
    mz_bze_bits W;
    uint32_t ip = 0, combined = 0, crc = 0;
    W.out = out;
    W.out_cap = out_cap;
    W.o = 0;
    W.wn = 0;
    W.cnt = 0;
    W.fail = 0;
    W.acc = 0;

    MZ_LANES {
        for (uint32_t k = 0; k < 4u; k++) { /* the block CRC's table: MSB-first, polynomial 0x04C11DB7 */
            uint32_t c = (4u * (uint32_t)lane + k) << 24;
            for (int b = 0; b < 8; b++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
            S->bzcrc[4u * (uint32_t)lane + k] = c;
        }
        for (uint32_t k = 0; k < MZ_BZE_WIN / 64u; k++) S->win[(uint32_t)lane + 64u * k] = 0u;
    }
    MZ_WAVE_SYNC();
    MZ_BZE_PUT(24, 0x425A68u); /* "BZh" */
    MZ_BZE_PUT(8, 0x30u + level);

    while (ip < in_len && !W.fail) {
        uint32_t n = 0, rb = 256u, rl = 0, cut = 0, bcrc = 0xFFFFFFFFu, ngroups = 0, nbits = 1, orig = 0, nuse = 0, nm = 0, alpha, ng, nsel;
        const uint32_t bs = ip;
        uint32_t *sa = A0, *sa2 = A1, *rk = R0, *rk2 = R1;
        uint64_t u0, u1, u2, u3;

        /* ---- 1. the first run-length stage and the block cut */
        while (ip < in_len && !cut) {
            PV(uint32_t, c);
            PV(uint32_t, nx);
            PV(uint32_t, st);
            PV(uint32_t, d);
            PV(uint32_t, e);
            PV(uint32_t, lit);
            PV(uint32_t, ce);
            PV(uint32_t, open);
            PV(uint32_t, em);
            PV(uint32_t, incl);
            uint64_t sm, okm;
            const uint32_t nvalid = in_len - ip < 64u ? in_len - ip : 64u;
            uint32_t take, last;
            MZ_LANES {
                const uint32_t i = ip + (uint32_t)lane;
                uint32_t cc = 256u, nn = 256u, pv = rb;
                if ((uint32_t)lane < nvalid) {
                    cc = in[i];
                    if (i + 1u < in_len) nn = in[i + 1u];
                    if (lane > 0) pv = in[i - 1u];
                }
                P(c) = cc;
                P(nx) = nn;
                P(st) = (uint32_t)lane < nvalid && cc != pv;
            }
            MZ_BALLOT(sm, P(st));
            MZ_LANES {
                const uint64_t mm = sm & (((uint64_t)2 << lane) - 1ull);
                const uint32_t dd = mm ? (uint32_t)lane - (63u - mz_clz64(mm)) : rl + (uint32_t)lane; /* place in the run of equal bytes */
                const uint32_t ee = dd % 255u;                                                       /* ... in the run as it is coded */
                const uint32_t nat = P(nx) != P(c) || ee == 254u;
                P(d) = dd;
                P(e) = ee;
                P(lit) = ee < 4u;
                P(ce) = nat && ee >= 3u;
                P(open) = !nat && ee >= 3u; /* ending the block here costs a count byte more */
                P(em) = (uint32_t)lane < nvalid ? P(lit) + P(ce) : 0u;
            }
            MZ_INCL_SCAN(incl, em);
            MZ_BALLOT(okm, (uint32_t)lane < nvalid && n + P(incl) + P(open) <= bmax);
            take = mz_popc64(okm); /* (the total never falls from one byte to the next: the mask has no holes) */
            if (take == 0) break;
            last = take - 1u;
            MZ_LANES {
                if ((uint32_t)lane < take) {
                    const uint32_t base = n + P(incl) - P(em);
                    if (P(lit)) blk[base] = (uint8_t)P(c);
                    if (P(ce) || ((uint32_t)lane == last && take < nvalid && P(open))) blk[base + P(lit)] = (uint8_t)(P(e) - 3u);
                }
            }
            n += MZ_READLANE(incl, last) + (take < nvalid ? MZ_READLANE(open, last) : 0u);
            rb = MZ_READLANE(c, last);
            rl = MZ_READLANE(d, last) + 1u;
            ip += take;
            if (take < nvalid) cut = 1;
        }
        /* the block CRC over in[bs, ip): a strip per lane, joined; the rest behind the strips byte by byte */
        {
            const uint32_t blen = ip - bs, strip = blen / 64u;
            PV(uint32_t, reg);
            PV(uint32_t, tb);
            MZ_LANES {
                uint32_t r = (lane == 0) ? 0xFFFFFFFFu : 0u;
                const uint8_t *q = in + bs + (size_t)lane * strip;
                const uint32_t t = bs + 64u * strip + (uint32_t)lane;
                for (uint32_t k = 0; k < strip; k++) r = (r << 8) ^ S->bzcrc[(r >> 24) ^ q[k]];
                P(reg) = r;
                P(tb) = t < ip ? in[t] : 0u;
            }
            if (strip) {
                uint32_t mul = 1u, sq = 2u;
                for (uint32_t ex = 8u * strip; ex; ex >>= 1) {
                    if (ex & 1u) mul = mz_bze_gfmul(mul, sq);
                    sq = mz_bze_gfmul(sq, sq);
                }
                bcrc = MZ_READLANE(reg, 0);
                for (uint32_t l = 1; l < 64u; l++) bcrc = mz_bze_gfmul(bcrc, mul) ^ MZ_READLANE(reg, l);
            }
            for (uint32_t k = 0; k < blen - 64u * strip; k++) bcrc = (bcrc << 8) ^ MZ_UNIFORM(S->bzcrc[(bcrc >> 24) ^ MZ_READLANE(tb, k)]);
            bcrc = ~bcrc;
            combined = ((combined << 1) | (combined >> 31)) ^ bcrc;
        }

        /* ---- 2. the rotations sorted.  First by the first byte: counts, starts, a stable scatter */
        MZ_LANES {
            for (uint32_t k = 0; k < 4u; k++) S->hist[4u * (uint32_t)lane + k] = 0;
        }
        MZ_CHASE_FENCE(); /* the symbols were stored a lane each and are read through other lanes from here on */
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t i = (uint32_t)lane; i < n; i += 64u) MZ_LDS_ATOMIC_INC(&S->hist[blk[i]]);
        }
        MZ_WAVE_SYNC();
        {
            PV(uint32_t, tot);
            PV(uint32_t, incl);
            PV(uint32_t, nz);
            MZ_LANES {
                const uint32_t *q = &S->hist[4u * (uint32_t)lane];
                P(tot) = q[0] + q[1] + q[2] + q[3];
                P(nz) = (q[0] != 0u) + (q[1] != 0u) + (q[2] != 0u) + (q[3] != 0u);
            }
            MZ_INCL_SCAN(incl, tot);
            MZ_WAVE_SUM(nuse, nz);
            MZ_BALLOT(u0, S->hist[4u * (uint32_t)lane] != 0u);
            MZ_BALLOT(u1, S->hist[4u * (uint32_t)lane + 1u] != 0u);
            MZ_BALLOT(u2, S->hist[4u * (uint32_t)lane + 2u] != 0u);
            MZ_BALLOT(u3, S->hist[4u * (uint32_t)lane + 3u] != 0u);
            MZ_LANES {
                const uint32_t *q = &S->hist[4u * (uint32_t)lane];
                uint32_t ex = P(incl) - P(tot);
                for (uint32_t k = 0; k < 4u; k++) {
                    S->start[4u * (uint32_t)lane + k] = ex;
                    S->start0[4u * (uint32_t)lane + k] = ex;
                    ex += q[k];
                }
            }
        }
        MZ_WAVE_SYNC();
        ngroups = nuse;
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            PV(uint32_t, byt);
            PV(uint32_t, last);
            PV(uint32_t, same);
            uint64_t valid, bal[8];
            MZ_LANES {
                const uint32_t i = i0 + (uint32_t)lane;
                P(byt) = i < n ? blk[i] : 0u;
            }
            MZ_BALLOT(valid, i0 + (uint32_t)lane < n);
            MZ_BALLOT(bal[0], P(byt) & 1u);
            MZ_BALLOT(bal[1], P(byt) & 2u);
            MZ_BALLOT(bal[2], P(byt) & 4u);
            MZ_BALLOT(bal[3], P(byt) & 8u);
            MZ_BALLOT(bal[4], P(byt) & 16u);
            MZ_BALLOT(bal[5], P(byt) & 32u);
            MZ_BALLOT(bal[6], P(byt) & 64u);
            MZ_BALLOT(bal[7], P(byt) & 128u);
            MZ_LANES {
                const uint32_t i = i0 + (uint32_t)lane, b = P(byt);
                uint64_t m = valid;
                for (uint32_t k = 0; k < 8u; k++) m &= ((b >> k) & 1u) ? bal[k] : ~bal[k];
                const uint32_t below = MZ_RANK_BELOW(m), n_same = mz_popc64(m);
                P(last) = 0;
                P(same) = n_same;
                if (i < n) {
                    sa[S->start[b] + below] = i; /* < n: the counts sum to n */
                    rk[i] = S->start0[b];
                    P(last) = below + 1u == n_same;
                }
            }
            MZ_WAVE_SYNC();
            MZ_LANES {
                if (P(last)) S->start[P(byt)] += P(same);
            }
            MZ_WAVE_SYNC();
        }
        MZ_CHASE_FENCE();
        MZ_WAVE_SYNC();
        while ((1u << nbits) < n) nbits++; /* ranks are below n */

        /* ... then prefix doubling: sa is ordered by the first h bytes, rk[i] = where the group of rotation i starts */
        for (uint32_t h = 1; ngroups < n && h < n; h <<= 1) {
            uint32_t carry = 0;
            MZ_LANES {
                for (uint32_t i = (uint32_t)lane; i < n; i += 64u) rk2[i] = 0u; /* the groups' fill counts */
            }
            MZ_CHASE_FENCE();
            MZ_WAVE_SYNC();
            for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
                PV(uint32_t, key);
                PV(uint32_t, idx);
                PV(uint32_t, cv);
                PV(uint32_t, last);
                PV(uint32_t, same);
                PV(uint64_t, m);
                uint64_t valid;
                MZ_LANES {
                    const uint32_t k = k0 + (uint32_t)lane;
                    P(key) = 0;
                    P(idx) = 0;
                    P(cv) = 0;
                    if (k < n) {
                        const uint32_t j = sa[k], i = j >= h ? j - h : j + n - h;
                        P(idx) = i;
                        P(key) = rk[i];
                        P(cv) = rk2[P(key)];
                    }
                }
                MZ_BALLOT(valid, k0 + (uint32_t)lane < n);
                MZ_LANES { P(m) = valid; }
                for (uint32_t b = 0; b < nbits; b++) {
                    uint64_t t;
                    MZ_BALLOT(t, (P(key) >> b) & 1u);
                    MZ_LANES { P(m) &= ((P(key) >> b) & 1u) ? t : ~t; }
                }
                MZ_LANES {
                    const uint32_t k = k0 + (uint32_t)lane, below = MZ_RANK_BELOW(P(m)), n_same = mz_popc64(P(m));
                    P(last) = 0;
                    P(same) = n_same;
                    if (k < n) {
                        sa2[P(key) + P(cv) + below] = P(idx); /* inside the group: its fill count never passes its size */
                        P(last) = below + 1u == n_same;
                    }
                }
                MZ_WAVE_SYNC();
                MZ_LANES {
                    if (P(last)) rk2[P(key)] = P(cv) + P(same);
                }
                MZ_CHASE_FENCE();
                MZ_WAVE_SYNC();
            }
            /* the new ranks (rk2 is free again: the counts are spent) */
            ngroups = 0;
            for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
                PV(uint32_t, bd);
                PV(uint32_t, ii);
                uint64_t bm;
                MZ_LANES {
                    const uint32_t k = k0 + (uint32_t)lane;
                    uint32_t bnd = 0, i = 0;
                    if (k < n) {
                        i = sa2[k];
                        if (k == 0) {
                            bnd = 1;
                        } else {
                            const uint32_t p = sa2[k - 1u];
                            if (rk[i] != rk[p]) {
                                bnd = 1;
                            } else {
                                const uint32_t i2 = i + h >= n ? i + h - n : i + h, p2 = p + h >= n ? p + h - n : p + h;
                                bnd = rk[i2] != rk[p2];
                            }
                        }
                    }
                    P(bd) = bnd;
                    P(ii) = i;
                }
                MZ_BALLOT(bm, P(bd));
                MZ_LANES {
                    const uint32_t k = k0 + (uint32_t)lane;
                    if (k < n) {
                        const uint64_t mm = bm & (((uint64_t)2 << lane) - 1ull);
                        rk2[P(ii)] = mm ? k0 + 63u - mz_clz64(mm) : carry;
                    }
                }
                if (bm) carry = k0 + 63u - mz_clz64(bm);
                ngroups += mz_popc64(bm);
            }
            MZ_CHASE_FENCE();
            MZ_WAVE_SYNC();
            {
                uint32_t *t = sa;
                sa = sa2;
                sa2 = t;
                t = rk;
                rk = rk2;
                rk2 = t;
            }
        }

        /* ---- 3. move-to-front over the last column; the list starts as the used byte values in order */
        {
            PV(uint32_t, nz);
            PV(uint32_t, incl);
            MZ_LANES {
                const uint32_t *q = &S->hist[4u * (uint32_t)lane];
                P(nz) = (q[0] != 0u) + (q[1] != 0u) + (q[2] != 0u) + (q[3] != 0u);
                for (uint32_t k = 0; k < 4u; k++) S->mtf[4u * (uint32_t)lane + k] = 0;
            }
            MZ_INCL_SCAN(incl, nz);
            MZ_WAVE_SYNC();
            MZ_LANES {
                const uint32_t *q = &S->hist[4u * (uint32_t)lane];
                uint32_t p = P(incl) - P(nz);
                for (uint32_t k = 0; k < 4u; k++)
                    if (q[k]) S->mtf[p++] = (uint8_t)(4u * (uint32_t)lane + k);
                for (uint32_t k = (uint32_t)lane; k < MZ_BZE_ALPHA + 2u; k += 64u) S->mfreq[k] = 0;
            }
            MZ_WAVE_SYNC();
        }
        {
            uint32_t front = MZ_UNIFORM(S->mtf[0]), zrun = 0;
            for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
                PV(uint32_t, lv);
                uint64_t zm;
                const uint32_t cnt = n - k0 < 64u ? n - k0 : 64u;
                MZ_LANES {
                    const uint32_t k = k0 + (uint32_t)lane;
                    uint32_t j = k < n ? sa[k] : 1u;
                    P(lv) = k < n ? blk[j ? j - 1u : n - 1u] : 0u;
                    P(lv) |= (k < n && j == 0u) ? 256u : 0u;
                }
                MZ_BALLOT(zm, P(lv) & 256u);
                if (zm) orig = k0 + mz_ctz64(zm);
                for (uint32_t q = 0; q < cnt; q++) {
                    const uint32_t b = MZ_READLANE(lv, q) & 255u;
                    uint32_t pos, fl;
                    uint64_t hit;
                    PV(uint32_t, hp);
                    if (b == front) {
                        zrun++;
                        continue;
                    }
                    while (zrun) { /* the run in bijective base 2: RUNA = 1, RUNB = 2 */
                        mtfv[nm++] = (uint16_t)((zrun & 1u) ? 0u : 1u);
                        zrun = (zrun - ((zrun & 1u) ? 1u : 2u)) >> 1;
                    }
                    MZ_LANES {
                        const uint32_t w = mz_ld4(&S->mtf[4 * lane]);
                        uint32_t p = 0xFFFFu;
                        if (((w >> 24) & 255u) == b) p = 4u * (uint32_t)lane + 3u;
                        if (((w >> 16) & 255u) == b) p = 4u * (uint32_t)lane + 2u;
                        if (((w >> 8) & 255u) == b) p = 4u * (uint32_t)lane + 1u;
                        if ((w & 255u) == b) p = 4u * (uint32_t)lane;
                        P(hp) = p;
                    }
                    MZ_BALLOT(hit, P(hp) != 0xFFFFu);
                    fl = mz_ctz64(hit | (1ull << 63)); /* (the byte is in the list: it occurs in the block) */
                    pos = MZ_READLANE(hp, fl) & 255u;
                    /* the list moves up by one in front of pos, the highest 64 positions first */
                    for (uint32_t j0 = (pos - 1u) & ~63u;; j0 -= 64u) {
                        PV(uint32_t, v);
                        MZ_LANES {
                            const uint32_t j = j0 + (uint32_t)lane;
                            P(v) = j < pos ? S->mtf[j] : 0u;
                        }
                        MZ_WAVE_SYNC();
                        MZ_LANES {
                            const uint32_t j = j0 + (uint32_t)lane;
                            if (j < pos) S->mtf[j + 1u] = (uint8_t)P(v);
                        }
                        MZ_WAVE_SYNC();
                        if (j0 == 0) break;
                    }
                    S->mtf[0] = (uint8_t)b;
                    MZ_WAVE_SYNC();
                    front = b;
                    mtfv[nm++] = (uint16_t)(pos + 1u); /* wave-uniform store */
                }
            }
            while (zrun) {
                mtfv[nm++] = (uint16_t)((zrun & 1u) ? 0u : 1u);
                zrun = (zrun - ((zrun & 1u) ? 1u : 2u)) >> 1;
            }
            mtfv[nm++] = (uint16_t)(nuse + 1u); /* end of block */
        }
        alpha = nuse + 2u;
        MZ_CHASE_FENCE(); /* the symbols were stored through one address per step and are read a lane per position */
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t i = (uint32_t)lane; i < nm; i += 64u) MZ_LDS_ATOMIC_INC(&S->mfreq[mtfv[i]]);
        }
        MZ_WAVE_SYNC();

        /* ---- 4. the tables */
        ng = nm < 200u ? 2u : nm < 600u ? 3u : nm < 1200u ? 4u : nm < 2400u ? 5u : 6u;
        nsel = (nm + MZ_BZE_G - 1u) / MZ_BZE_G;
        {
            uint32_t rem = nm, gs = 0;
            for (uint32_t part = ng; part > 0; part--) { /* libbz2's first partition: symbol ranges of about equal frequency */
                const uint32_t tf = rem / part;
                uint32_t af = 0;
                int32_t ge = (int32_t)gs - 1;
                while (af < tf && ge < (int32_t)alpha - 1) {
                    ge++;
                    af += MZ_UNIFORM(S->mfreq[ge]);
                }
                if (ge > (int32_t)gs && part != ng && part != 1u && ((ng - part) & 1u)) {
                    af -= MZ_UNIFORM(S->mfreq[ge]);
                    ge--;
                }
                MZ_LANES {
                    for (uint32_t v = (uint32_t)lane; v < alpha; v += 64u) S->len[part - 1u][v] = ((int32_t)v >= (int32_t)gs && (int32_t)v <= ge) ? 0u : 15u;
                }
                gs = (uint32_t)(ge + 1);
                rem -= af;
            }
        }
        MZ_WAVE_SYNC();
        for (uint32_t it = 0; it < MZ_BZE_ITERS; it++) {
            MZ_LANES {
                for (uint32_t v = (uint32_t)lane; v < alpha; v += 64u) {
                    uint64_t pk = 0;
                    for (uint32_t t = 0; t < ng; t++) {
                        pk |= (uint64_t)S->len[t][v] << (10u * t);
                        S->rfreq[t][v] = 0;
                    }
                    S->lenpack[v] = pk;
                }
            }
            MZ_WAVE_SYNC();
            for (uint32_t g0 = 0; g0 < nsel; g0 += 64u) {
                PV(uint32_t, bt);
                MZ_LANES {
                    const uint32_t g = g0 + (uint32_t)lane;
                    P(bt) = 0;
                    if (g < nsel) {
                        const uint32_t i0 = g * MZ_BZE_G, i1 = i0 + MZ_BZE_G < nm ? i0 + MZ_BZE_G : nm;
                        uint64_t cost = 0;
                        uint32_t best = 0, bc;
                        for (uint32_t i = i0; i < i1; i++) cost += S->lenpack[mtfv[i]];
                        bc = (uint32_t)cost & 1023u;
                        for (uint32_t t = 1; t < ng; t++) {
                            const uint32_t c = (uint32_t)(cost >> (10u * t)) & 1023u;
                            if (c < bc) {
                                bc = c;
                                best = t;
                            }
                        }
                        P(bt) = best;
                        sel[g] = (uint8_t)best;
                    }
                }
                MZ_WAVE_SYNC();
                MZ_LANES {
                    const uint32_t g = g0 + (uint32_t)lane;
                    if (g < nsel) {
                        const uint32_t i0 = g * MZ_BZE_G, i1 = i0 + MZ_BZE_G < nm ? i0 + MZ_BZE_G : nm;
                        for (uint32_t i = i0; i < i1; i++) MZ_LDS_ATOMIC_INC(&S->rfreq[P(bt)][mtfv[i]]);
                    }
                }
                MZ_WAVE_SYNC();
            }
            for (uint32_t t = 0; t < ng; t++) mz_bze_make_lengths(S, S->rfreq[t], S->len[t], alpha);
        }
        MZ_CHASE_FENCE(); /* the selectors were stored a lane per group and are read a lane per symbol */
        MZ_WAVE_SYNC();
        for (uint32_t t = 0; t < ng; t++) {
            PV(uint32_t, c1);
            PV(uint32_t, c2);
            uint32_t cost, flat, vec = 0;
            MZ_LANES {
                P(c1) = 0;
                P(c2) = 0;
                for (uint32_t v = (uint32_t)lane; v < alpha; v += 64u) {
                    P(c1) += S->rfreq[t][v] * S->len[t][v];
                    P(c2) += S->rfreq[t][v] * mz_bze_flat_len(v, alpha);
                }
                if (lane < 24) S->lcount[lane] = 0;
            }
            MZ_WAVE_SUM(cost, c1);
            MZ_WAVE_SUM(flat, c2);
            MZ_WAVE_SYNC();
            if (cost > flat) { /* never worse than the flat code: the output bound rests on it */
                MZ_LANES {
                    for (uint32_t v = (uint32_t)lane; v < alpha; v += 64u) S->len[t][v] = (uint8_t)mz_bze_flat_len(v, alpha);
                }
                MZ_WAVE_SYNC();
            }
            /* the codes as BZ2_hbAssignCodes numbers them: by length, then by symbol */
            MZ_LANES {
                for (uint32_t v = (uint32_t)lane; v < alpha; v += 64u) MZ_LDS_ATOMIC_INC(&S->lcount[S->len[t][v]]);
            }
            MZ_WAVE_SYNC();
            for (uint32_t l = 1; l <= MZ_BZE_MAXLEN; l++) {
                S->fcode[l] = vec;
                vec = (vec + MZ_UNIFORM(S->lcount[l])) << 1;
            }
            MZ_WAVE_SYNC();
            MZ_LANES {
                for (uint32_t v = (uint32_t)lane; v < alpha; v += 64u) {
                    const uint32_t l = S->len[t][v];
                    uint32_t c = 0;
                    for (uint32_t j = 0; j < v; j++) c += S->len[t][j] == l;
                    S->code[t][v] = S->fcode[l] + c;
                }
            }
            MZ_WAVE_SYNC();
        }

        /* ---- 5. the block written */
        MZ_BZE_PUT(24, 0x314159u);
        MZ_BZE_PUT(24, 0x265359u);
        MZ_BZE_PUT(32, bcrc);
        MZ_BZE_PUT(1, 0u); /* not randomised */
        MZ_BZE_PUT(24, orig);
        {
            uint32_t m16 = 0;
            for (uint32_t g = 0; g < 16u; g++)
                if (((u0 | u1 | u2 | u3) >> (4u * g)) & 15u) m16 |= 1u << (15u - g);
            MZ_BZE_PUT(16, m16);
            for (uint32_t g = 0; g < 16u; g++) {
                uint32_t w16 = 0;
                if (!((m16 >> (15u - g)) & 1u)) continue;
                for (uint32_t j = 0; j < 16u; j++) {
                    const uint64_t u = (j & 3u) == 0u ? u0 : (j & 3u) == 1u ? u1 : (j & 3u) == 2u ? u2 : u3;
                    if ((u >> (4u * g + (j >> 2))) & 1u) w16 |= 1u << (15u - j);
                }
                MZ_BZE_PUT(16, w16);
            }
        }
        MZ_BZE_PUT(3, ng);
        MZ_BZE_PUT(15, nsel);
        {
            uint32_t lst = 0x543210u; /* the selectors' move-to-front list: six nibbles */
            for (uint32_t g0 = 0; g0 < nsel; g0 += 64u) {
                PV(uint32_t, sv);
                const uint32_t cnt = nsel - g0 < 64u ? nsel - g0 : 64u;
                MZ_LANES { P(sv) = g0 + (uint32_t)lane < nsel ? sel[g0 + (uint32_t)lane] : 0u; }
                for (uint32_t q = 0; q < cnt; q++) {
                    const uint32_t v = MZ_READLANE(sv, q);
                    uint32_t j = 0, low;
                    while (((lst >> (4u * j)) & 15u) != v) j++;
                    low = lst & ((1u << (4u * j)) - 1u);
                    lst = (lst & ~((1u << (4u * j + 4u)) - 1u)) | (low << 4) | v;
                    MZ_BZE_PUT(j + 1u, ((1u << j) - 1u) << 1);
                }
            }
        }
        for (uint32_t t = 0; t < ng; t++) {
            uint32_t curr = MZ_UNIFORM(S->len[t][0]);
            MZ_BZE_PUT(5, curr);
            for (uint32_t v = 0; v < alpha; v++) {
                const uint32_t l = MZ_UNIFORM(S->len[t][v]);
                while (curr < l) {
                    MZ_BZE_PUT(2, 2u);
                    curr++;
                }
                while (curr > l) {
                    MZ_BZE_PUT(2, 3u);
                    curr--;
                }
                MZ_BZE_PUT(1, 0u);
            }
        }
        /* the symbols, 64 per step; the pending bits go to the window first and come back behind the last step */
        S->win[W.wn] = W.cnt ? (uint32_t)(W.acc << (32u - W.cnt)) : 0u;
        MZ_WAVE_SYNC();
        for (uint32_t i0 = 0; i0 < nm; i0 += 64u) {
            PV(uint32_t, cl);
            PV(uint32_t, cd);
            PV(uint32_t, incl);
            uint32_t base, np;
            if (W.wn + 36u > MZ_BZE_WIN) mz_bze_flush(&W, S); /* 64 codes of 17 bits behind 31 pending ones: 35 words */
            MZ_LANES {
                const uint32_t i = i0 + (uint32_t)lane;
                P(cl) = 0;
                P(cd) = 0;
                if (i < nm) {
                    const uint32_t s = mtfv[i], t = sel[i / MZ_BZE_G];
                    P(cl) = S->len[t][s];
                    P(cd) = S->code[t][s];
                }
            }
            MZ_INCL_SCAN(incl, cl);
            base = 32u * W.wn + W.cnt;
            MZ_LANES {
                const uint32_t l = P(cl);
                if (l) {
                    const uint32_t off = base + P(incl) - l, w = off >> 5, b = off & 31u;
                    if (b + l <= 32u) {
                        MZ_LDS_ATOMIC_OR(&S->win[w], P(cd) << (32u - b - l));
                    } else {
                        MZ_LDS_ATOMIC_OR(&S->win[w], P(cd) >> (b + l - 32u));
                        MZ_LDS_ATOMIC_OR(&S->win[w + 1u], P(cd) << (64u - b - l));
                    }
                }
            }
            np = base + MZ_READLANE(incl, 63);
            W.wn = np >> 5;
            W.cnt = np & 31u;
            MZ_WAVE_SYNC();
        }
        W.acc = W.cnt ? (uint64_t)(MZ_UNIFORM(S->win[W.wn]) >> (32u - W.cnt)) : 0ull;
        MZ_WAVE_SYNC();
        S->win[W.wn] = 0u;
        MZ_WAVE_SYNC();
    }

    /* the stream's end: 0x177245385090, the combined CRC, padding to a byte */
    MZ_BZE_PUT(24, 0x177245u);
    MZ_BZE_PUT(24, 0x385090u);
    MZ_BZE_PUT(32, combined);
    mz_bze_flush(&W, S);
    {
        const uint32_t nb = (W.cnt + 7u) / 8u, top = W.cnt ? (uint32_t)(W.acc << (32u - W.cnt)) : 0u;
        if (nb > W.out_cap - W.o) W.fail = 1u;
        if (!W.fail) {
            for (uint32_t k = 0; k < nb; k++) out[W.o + k] = (uint8_t)(top >> (24u - 8u * k)); /* wave-uniform stores */
            W.o += nb;
        }
    }

    /* the ZIP CRC-32 of the input: the K2 fold */
    MZ_WAVE_SYNC();
    {
        PV(uint32_t, acc);
        PV(uint32_t, tmp);
        uint32_t folded = 0;
        MZ_LANES { P(acc) = (lane == 0) ? 0xFFFFFFFFu : 0u; }
        MZ_CRC_FOLD_TILES(acc, folded, in, in_len, crc_tab, tabs->kx);
        MZ_CRC_FINISH(crc, acc, tmp, folded, in, in_len, crc_tab, tabs);
    }
    res->out_len = W.fail ? 0u : W.o;
    res->crc = crc;
    res->status = W.fail ? MZHIP_OUT_FULL : MZHIP_OK;
}

#endif
