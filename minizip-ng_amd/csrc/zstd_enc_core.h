/* zstd_enc_core.h -- one Zstandard frame (ZIP method 93, RFC 8878; the reference's mz_strm_zstd.c over ZSTD_compressStream2)
 * written by one wave from the LZ77 tokens of lzma_enc_core.h.
 *
 * Written in the wave.h vocabulary: the same text is the gfx950 kernel body (k_zstd_encode_batch) and, under
 * g++ -DMZHIP_HOST_EMUL, the host build the CPU tests run (tests/emul/emul_zstd_enc.cpp).  No decision uses floating point:
 * costs are sums of mz_zse_log2fp (an integer log2 with 8 fractional bits from the 64-entry table below), so the device's
 * bytes are the emulation's.  The bytes are valid Zstandard but not libzstd's: parity is "ZSTD_decompress returns the input".
 *
 * The parse is K6's (mz_lz_chain, mz_lz_tokenize, launched before this kernel): per 64 KiB block literals and matches of
 * length 4 .. 273, distance <= 32 KiB in a stream of one block and < MZ_LZE_FAR_DICT beyond.  One Zstandard block per parse
 * block.  Per block the wave
 *   1. turns tokens into sequences, 64 tokens per step: a scan gives every literal its place in the literal buffer (scratch)
 *      and every match that does not go on the match in front of it (same distance, no literal between) its sequence index;
 *      a run of such matches is ONE sequence, its length the segmented sum of the run (the last sequence of a step stays
 *      open in registers, the next step may lengthen it);
 *   2. resolves the repeat offsets in stream order (1, 4, 8 at the frame's start, carried over the frame's blocks, restored
 *      when the block goes out Raw or RLE): 64 records are loaded by the lanes, the serial part reads them from registers.
 *      Offset values 1 .. 3 are used wherever they name the distance, with their shifted meaning when the literal length is
 *      0.  The same pass derives the LL / ML / OF codes and their histograms (LDS atomics);
 *   3. codes the literals: histogram in LDS; one value = RLE; else a Huffman code of at most 11 bits (two queues over the
 *      sorted counts, the counts halved until no code is longer: always a complete code whose two longest codes are
 *      siblings), described directly or with FSE-compressed weights (needed from byte 128 on; taken when legal and
 *      shorter), 1 stream up to 1023 literals and 4 beyond; Raw when that is not smaller or cannot be described.  All 64
 *      lanes code: a stream is written from its last symbol to its first, a scan over the code lengths gives the bit offsets,
 *      the codes are OR-ed into an LDS window, the closing 1-bit follows;
 *   4. chooses per table the cheapest of Predefined, RLE (one occurring code) and FSE_Compressed (counts normalised by
 *      rounding, the difference to the table size taken by the most probable code; accuracy log from the sequence count,
 *      5 .. 9, offsets 5 .. 8) by mz_zse_log2fp cost including the description, and walks the three FSE states backward over
 *      the sequences, wave-uniform, 64 sequences prepared by the lanes per step, through the same LDS window;
 *   5. takes the block Compressed when that is smaller than its bytes, RLE when its bytes are all equal, Raw otherwise.
 * The frame: magic, Single_Segment with the smallest Frame_Content_Size field up to MZ_LZE_FAR_DICT bytes, beyond a
 * Window_Descriptor of exactly 8 MiB and a 4-byte content size; no dictionary id; flags bit 0 = XXH64 content checksum.
 * Repeat and Treeless modes are never written: a block depends on the blocks before it through the repeat offsets only.
 *
 * LDS: sizeof(mz_zse_lds) = 14 928 bytes per wave (with the kernel's CRC table 15 952: 10 single-wave workgroups would fit a
 * CU's 160 KiB; the launch keeps 8, which is also what the registers allow).  Scratch in HBM per resident wave:
 * MZ_ZSE_SCRATCH_BYTES = 263 168 -- 64 KiB of literals, 16 384 sequence records of 8 bytes (a block of 64 KiB holds at most
 * 16 384 matches of 4 bytes), 65 KiB in which the block's body is staged before the block type is known.
 * Compiler's remarks (profiles/zstd/resource_usage_enc.txt): 253 VGPRs, no private scratch, 2 waves per SIMD.
 */
#ifndef MZHIP_ZSTD_ENC_CORE_H
#define MZHIP_ZSTD_ENC_CORE_H

#include "lzma_enc_core.h"
#include "zstd_core.h"

#define MZ_ZSE_MAXSEQ 16384u
#define MZ_ZSE_STAGE_BYTES (MZ_DEF_BLOCK + 1024u)
#define MZ_ZSE_SCRATCH_BYTES (MZ_DEF_BLOCK + 8u * MZ_ZSE_MAXSEQ + MZ_ZSE_STAGE_BYTES)
#define MZ_ZSE_WIN 256u /* words of the bit window */
#define MZ_ZSE_HUF_MAX 11u

/* level as mz_strm_zstd.c hands it to ZSTD_c_compressionLevel: -1 and 0 mean 3; 1 .. 22 */
#define MZ_ZSE_LEVEL_OK(level) ((level) >= -1 && (level) <= 22)
/* the class of the parse as an LZMA preset (set_lz_class): levels 1-2 one way and one far link, 3-6 MZ_DEF_WAYS_BEST ways and 4
 * links, 7-15 8 links, 16-22 16 links */
#define MZ_ZSE_PRESET(level) (((level) <= 0) ? 4 : ((level) <= 2) ? 0 : ((level) <= 6) ? 4 : ((level) <= 15) ? 6 : 9)
/* An output size that always suffices: 10 bytes of frame header at the most (magic, descriptor, window byte or not, 4 bytes
 * of content size), per 64 KiB block begun (one for an empty input) a 3-byte header and never more than the block's bytes
 * (a Compressed block is taken only when it is smaller, an RLE block holds one byte), 4 bytes of checksum. */
#define MZ_ZSE_BOUND(in_len) (14ull + (uint64_t)(in_len) + 3ull * ((in_len) ? ((uint64_t)(in_len) + MZ_DEF_BLOCK - 1u) / MZ_DEF_BLOCK : 1ull))

/* 256 * log2(1 + i / 64), rounded */
MZ_ZS_TABLE uint8_t mz_zse_log2[64] = {0,   6,   11,  17,  22,  28,  33,  38,  44,  49,  54,  59,  63,  68,  73,  78,  82,  87,  92,  96,  100, 105,
                                       109, 113, 118, 122, 126, 130, 134, 138, 142, 146, 150, 154, 157, 161, 165, 169, 172, 176, 179, 183, 186, 190,
                                       193, 197, 200, 203, 207, 210, 213, 216, 220, 223, 226, 229, 232, 235, 238, 241, 244, 247, 250, 253};
/* log2(x) with 8 fractional bits, x >= 1 */
MZ_DEV uint32_t mz_zse_log2fp(uint32_t x) {
    const uint32_t hb = mz_zs_highbit(x);
    return (hb << 8) + mz_zse_log2[((x << (31u - hb)) >> 25) & 63u];
}

typedef struct mz_zse_lds {
    uint32_t win[MZ_ZSE_WIN];
    uint32_t hist[256];               /* the block's literals by value */
    uint32_t hf[256];                 /* Huffman: the counts as they are halved, */
    uint32_t hw[256];                 /* ... sorted (the leaves), */
    uint32_t hiw[256];                /* the inner nodes' weights in the order they are made */
    uint32_t shist[3][64];            /* LL / OF / ML codes of the block's sequences */
    uint32_t dnb[3][64];              /* FSE coding tables: deltaNbBits, */
    int32_t dfs[3][64];               /* deltaFindState, */
    uint16_t stt[3][512];             /* the next state */
    uint16_t hparent[512];
    uint16_t horder[256];
    uint16_t hcode[256];
    uint16_t cumul[64];
    int16_t norm[3][64];
    int16_t dnorm[64];
    uint32_t rank[16];
    uint32_t tmp[4];
    uint8_t hlen[256];
    uint8_t wts[256];
    uint8_t tsym[512];
    uint8_t desc[3][128]; /* the descriptions of the three tables */
    uint8_t wdesc[256];   /* the description of the Huffman tree */
} mz_zse_lds;

typedef struct mz_zse_result {
    uint32_t out_len; /* 0 unless the status is 0 */
    uint32_t crc;     /* CRC-32 of the input */
    int32_t status;
} mz_zse_result;

/* counters of the host emulation: the tests hold the bound of 16 384 sequences per block with them */
#if defined(MZHIP_HOST_EMUL)
static uint32_t mz_zse_max_nseq;
#define MZ_ZSE_NOTE_NSEQ(n) (mz_zse_max_nseq = (n) > mz_zse_max_nseq ? (n) : mz_zse_max_nseq)
#else
#define MZ_ZSE_NOTE_NSEQ(n) ((void)0)
#endif

/* measurement builds (make PROF=1): cycles of the stages, summed over all waves, in mz_prof_buf[27 .. 31] (the buffer has 32
 * words; the decoders' last ones are shared, one kernel is measured at a time): 27 sequence build and repeat offsets,
 * 28 histograms and tables, 29 literal coding, 30 sequence coding, 31 framing, copies, XXH64 and CRC-32 */
#if defined(MZ_PROF) && !defined(MZHIP_HOST_EMUL)
#define MZ_ZSEPROF_INIT uint32_t prof_acc = 0; uint64_t prof_t0 = __builtin_readcyclecounter();
#define MZ_ZSEPROF_MARK(i)                                                         \
    do {                                                                           \
        const uint32_t _pd = (uint32_t)(__builtin_readcyclecounter() - prof_t0);   \
        prof_acc += (lane == 27 + (i)) ? _pd : 0u;                                 \
        prof_t0 = __builtin_readcyclecounter();                                    \
    } while (0)
#define MZ_ZSEPROF_FLUSH if (lane >= 27 && lane < 32) atomicAdd(&mz_prof_buf[lane], (unsigned long long)prof_acc);
#else
#define MZ_ZSEPROF_INIT
#define MZ_ZSEPROF_MARK(i) ((void)0)
#define MZ_ZSEPROF_FLUSH
#endif

/* LSB-first bit writer into dst[0 .. cap): pending bits in acc (cnt < 32 of them), whole words in the window win[0 .. wn); every
 * word from wn on is zero, except while the lanes code symbols (then win[wn] holds the pending bits) */
typedef struct mz_zse_bits {
    uint8_t *dst;
    uint32_t cap, o, wn, cnt, fail;
    uint64_t acc;
} mz_zse_bits;

MZ_DEV void mz_zse_open(mz_zse_bits *W, mz_zse_lds *S, uint8_t *dst, uint32_t cap) {
    MZ_LANE_DECL
    W->dst = dst;
    W->cap = cap;
    W->o = 0;
    W->wn = 0;
    W->cnt = 0;
    W->fail = 0;
    W->acc = 0;
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < MZ_ZSE_WIN / 64u; k++) S->win[(uint32_t)lane + 64u * k] = 0u;
    }
    MZ_WAVE_SYNC();
}

/* the window's whole words to the output, the word behind them (pending bits or zero) to the front */
MZ_DEV void mz_zse_flush(mz_zse_bits *W, mz_zse_lds *S) {
    MZ_LANE_DECL
    const uint32_t wn = W->wn, need = 4u * wn;
    uint32_t part;
    MZ_WAVE_SYNC();
    if (need > W->cap - W->o) W->fail = 1u;
    if (!W->fail) {
        MZ_LANES {
            for (uint32_t w = (uint32_t)lane; w < wn; w += 64u) mz_st4(W->dst + W->o + 4u * w, S->win[w]);
        }
        W->o += need;
    }
    part = MZ_UNIFORM(S->win[wn]);
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < MZ_ZSE_WIN / 64u; k++) S->win[(uint32_t)lane + 64u * k] = 0u;
    }
    MZ_WAVE_SYNC();
    S->win[0] = part; /* wave-uniform: stored by all lanes */
    MZ_WAVE_SYNC();
    W->wn = 0;
}

/* n <= 32 bits, v < 2^n */
MZ_DEV void mz_zse_put(mz_zse_bits *W, mz_zse_lds *S, uint32_t n, uint32_t v) {
    W->acc |= (uint64_t)v << W->cnt;
    W->cnt += n;
    if (W->cnt >= 32u) {
        W->cnt -= 32u;
        S->win[W->wn] = (uint32_t)W->acc;
        W->wn++;
        W->acc >>= 32;
        if (W->wn + 2u >= MZ_ZSE_WIN) mz_zse_flush(W, S);
    }
}

/* the closing 1-bit, then everything to the output; -> the stream's bytes (0 and W->fail when it does not fit) */
MZ_DEV uint32_t mz_zse_close(mz_zse_bits *W, mz_zse_lds *S) {
    mz_zse_put(W, S, 1u, 1u);
    mz_zse_flush(W, S);
    {
        const uint32_t nb = (W->cnt + 7u) / 8u;
        if (nb > W->cap - W->o) W->fail = 1u;
        if (W->fail) return 0;
        for (uint32_t k = 0; k < nb; k++) W->dst[W->o + k] = (uint8_t)(W->acc >> (8u * k)); /* wave-uniform stores */
        W->o += nb;
    }
    MZ_WAVE_SYNC();
    S->win[0] = 0u;
    MZ_WAVE_SYNC();
    return W->o;
}

/* a small forward bit field in LDS (table descriptions, the compressed weights): LSB first */
typedef struct mz_zse_lbits {
    uint8_t *buf;
    uint32_t n, cnt;
    uint64_t acc;
} mz_zse_lbits;
MZ_DEV void mz_zse_lput(mz_zse_lbits *B, uint32_t nb, uint32_t v) {
    B->acc |= (uint64_t)v << B->cnt;
    B->cnt += nb;
    while (B->cnt >= 8u) {
        B->buf[B->n++] = (uint8_t)B->acc; /* wave-uniform store */
        B->acc >>= 8;
        B->cnt -= 8u;
    }
}
MZ_DEV void mz_zse_lpad(mz_zse_lbits *B) {
    if (B->cnt) mz_zse_lput(B, 8u - B->cnt, 0u);
}

MZ_DEV int32_t mz_zse_ld16(const int16_t *p) { return (int32_t)(int16_t)MZ_UNIFORM((uint32_t)(int32_t)*p); }

/* counts hist[0 .. nsym) (their sum: total; at most 1 << (al - 1) of them occur) -> norm[] that sums to 1 << al: rounded
 * shares, at least 1 for a code that occurs; the most probable code (the first of them) takes the difference */
MZ_DEV void mz_zse_normalize(const uint32_t *hist, uint32_t nsym, uint32_t total, uint32_t al, int16_t *norm) {
    const uint32_t T = 1u << al;
    uint32_t sum = 0;
    MZ_WAVE_SYNC();
    for (uint32_t s = 0; s < nsym; s++) {
        const uint32_t c = MZ_UNIFORM(hist[s]);
        uint32_t p = c ? (c * T + total / 2u) / total : 0u;
        if (c && !p) p = 1u;
        norm[s] = (int16_t)p;
        sum += p;
    }
    while (sum != T) {
        uint32_t best = 0, bp = 0;
        for (uint32_t s = 0; s < nsym; s++) {
            const uint32_t p = (uint32_t)mz_zse_ld16(&norm[s]);
            if (p > bp) {
                bp = p;
                best = s;
            }
        }
        if (sum < T) {
            norm[best] = (int16_t)(bp + (T - sum));
            sum = T;
        } else {
            const uint32_t take = sum - T < bp - 1u ? sum - T : bp - 1u; /* (bp > 1: fewer codes occur than the table has cells) */
            if (!take) break;
            norm[best] = (int16_t)(bp - take);
            sum -= take;
        }
    }
    MZ_WAVE_SYNC();
}

/* the description of norm[0 .. nsym) at accuracy log al (RFC 8878 4.1.1) into buf; -> its bytes */
MZ_DEV uint32_t mz_zse_ncount(const int16_t *norm, uint32_t nsym, uint32_t al, uint8_t *buf) {
    const uint32_t T = 1u << al;
    uint32_t acc = 0, s = 0;
    mz_zse_lbits B;
    B.buf = buf;
    B.n = 0;
    B.cnt = 0;
    B.acc = 0;
    mz_zse_lput(&B, 4u, al - 5u);
    while (acc < T && s < nsym) {
        const int32_t p = mz_zse_ld16(&norm[s]);
        const uint32_t rem1 = T - acc + 1u, nb = mz_zs_highbit(rem1) + 1u, lower = (1u << (nb - 1u)) - 1u, thr = (1u << nb) - 1u - rem1;
        const uint32_t val = (uint32_t)(p + 1);
        if (val < thr)
            mz_zse_lput(&B, nb - 1u, val);
        else
            mz_zse_lput(&B, nb, val > lower ? val + thr : val);
        acc += p < 0 ? 1u : (uint32_t)p;
        s++;
        if (p == 0) {
            uint32_t z = 0;
            while (s + z < nsym && mz_zse_ld16(&norm[s + z]) == 0) z++;
            s += z;
            while (z >= 3u) {
                mz_zse_lput(&B, 2u, 3u);
                z -= 3u;
            }
            mz_zse_lput(&B, 2u, z);
        }
    }
    mz_zse_lpad(&B);
    MZ_WAVE_SYNC();
    return B.n;
}

/* the coding table t of norm[0 .. nsym) at accuracy log al: the decoder's spread (mz_zs_fse_build), the states of a code in
 * cell order, and per code what a step shifts out and where it goes on */
MZ_DEV void mz_zse_ctable(mz_zse_lds *S, uint32_t t, const int16_t *norm, uint32_t nsym, uint32_t al) {
    const uint32_t T = 1u << al, mask = T - 1u, step = (T >> 1) + (T >> 3) + 3u;
    uint32_t high = T - 1u, pos = 0, cum = 0, total = 0;
    MZ_WAVE_SYNC();
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t p = mz_zse_ld16(&norm[s]);
        S->cumul[s] = (uint16_t)cum;
        if (p < 0) {
            S->tsym[high] = (uint8_t)s;
            high--;
            cum += 1u;
        } else {
            cum += (uint32_t)p;
        }
    }
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t p = mz_zse_ld16(&norm[s]);
        for (int32_t i = 0; i < p; i++) {
            S->tsym[pos] = (uint8_t)s;
            do pos = (pos + step) & mask;
            while (pos > high && high != 0xFFFFFFFFu);
        }
    }
    MZ_WAVE_SYNC();
    for (uint32_t u = 0; u < T; u++) {
        const uint32_t s = MZ_UNIFORM(S->tsym[u]) & 63u, c = MZ_UNIFORM(S->cumul[s]);
        S->stt[t][c & 511u] = (uint16_t)(T + u);
        S->cumul[s] = (uint16_t)(c + 1u);
    }
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t p = mz_zse_ld16(&norm[s]);
        if (p == 0) {
            S->dnb[t][s] = ((al + 1u) << 16) - T;
            S->dfs[t][s] = 0;
        } else if (p == -1 || p == 1) {
            S->dnb[t][s] = (al << 16) - T;
            S->dfs[t][s] = (int32_t)total - 1;
            total++;
        } else {
            const uint32_t mbo = al - mz_zs_highbit((uint32_t)p - 1u);
            S->dnb[t][s] = (mbo << 16) - ((uint32_t)p << mbo);
            S->dfs[t][s] = (int32_t)total - p;
            total += (uint32_t)p;
        }
    }
    MZ_WAVE_SYNC();
}

/* a state of table t that decodes `sym` and is left with the most bits (FSE_initCState2) */
MZ_DEV uint32_t mz_zse_state0(mz_zse_lds *S, uint32_t t, uint32_t sym) {
    const uint32_t d = MZ_UNIFORM(S->dnb[t][sym]), nb = (d + (1u << 15)) >> 16, value = (nb << 16) - d;
    return MZ_UNIFORM(S->stt[t][(uint32_t)((int32_t)(value >> nb) + (int32_t)MZ_UNIFORM((uint32_t)S->dfs[t][sym])) & 511u]);
}
/* what coding `sym` in front of `state` shifts out: *nb bits of *v; -> the state that decodes sym and goes on to `state` */
MZ_DEV uint32_t mz_zse_step(mz_zse_lds *S, uint32_t t, uint32_t state, uint32_t sym, uint32_t *nb, uint32_t *v) {
    const uint32_t n = (state + MZ_UNIFORM(S->dnb[t][sym])) >> 16;
    *nb = n;
    *v = state & ((1u << n) - 1u);
    return MZ_UNIFORM(S->stt[t][(uint32_t)((int32_t)(state >> n) + (int32_t)MZ_UNIFORM((uint32_t)S->dfs[t][sym])) & 511u]);
}

/* bits (8 fractional) that coding hist[0 .. nsym) with norm[] at accuracy log al takes; 0xFFFFFFFF if a code that occurs has
 * no cell */
MZ_DEV uint32_t mz_zse_cost(const uint32_t *hist, const int16_t *norm, uint32_t nsym, uint32_t al) {
    MZ_LANE_DECL
    PV(uint32_t, c);
    uint64_t bad;
    uint32_t sum;
    MZ_WAVE_SYNC();
    MZ_LANES {
        const uint32_t s = (uint32_t)lane;
        const uint32_t h = s < nsym ? hist[s] : 0u;
        const int32_t p = s < nsym ? (int32_t)norm[s] : 0;
        P(c) = (h && p) ? h * ((al << 8) - mz_zse_log2fp(p < 0 ? 1u : (uint32_t)p)) : 0u;
    }
    MZ_BALLOT(bad, (uint32_t)lane < nsym && hist[(uint32_t)lane < nsym ? (uint32_t)lane : 0u] != 0u && norm[(uint32_t)lane < nsym ? (uint32_t)lane : 0u] == 0);
    MZ_WAVE_SUM(sum, c);
    return bad ? 0xFFFFFFFFu : sum;
}

MZ_DEV uint32_t mz_zse_ll_code(uint32_t ll) {
    if (ll < 16u) return ll;
    if (ll < 24u) return 16u + ((ll - 16u) >> 1);
    if (ll < 32u) return 20u + ((ll - 24u) >> 2);
    if (ll < 48u) return 22u + ((ll - 32u) >> 3);
    if (ll < 64u) return 24u;
    return mz_zs_highbit(ll) + 19u;
}
/* mlb = match length - 3 */
MZ_DEV uint32_t mz_zse_ml_code(uint32_t mlb) {
    if (mlb < 32u) return mlb;
    if (mlb < 40u) return 32u + ((mlb - 32u) >> 1);
    if (mlb < 48u) return 36u + ((mlb - 40u) >> 2);
    if (mlb < 64u) return 38u + ((mlb - 48u) >> 3);
    if (mlb < 96u) return 40u + ((mlb - 64u) >> 4);
    if (mlb < 128u) return 42u;
    return mz_zs_highbit(mlb) + 36u;
}

/* Code lengths of at most MZ_ZSE_HUF_MAX bits for the values with S->hist != 0 (at least two) into S->hlen (0 elsewhere): the
 * values sorted by (count, value) with a lane per value, Huffman's tree by two queues (wave-uniform), depths by walking up,
 * a lane per leaf; while a code is too long the counts are halved (1 + f / 2) and the tree is made again.  -> the longest
 * length */
MZ_DEV uint32_t mz_zse_huf_lengths(mz_zse_lds *S) {
    MZ_LANE_DECL
    uint32_t nz, maxlen;
    PV(uint32_t, pc);
    MZ_WAVE_SYNC();
    MZ_LANES {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t s = (uint32_t)lane + 64u * k;
            S->hf[s] = S->hist[s];
            S->hlen[s] = 0;
            c += S->hist[s] != 0u;
        }
        P(pc) = c;
    }
    MZ_WAVE_SUM(nz, pc);
    for (;;) {
        uint32_t a = 0, b = 0;
        const uint32_t root = 2u * nz - 2u;
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t i = (uint32_t)lane + 64u * k, f = S->hf[i];
                if (f) {
                    uint32_t r = 0;
                    for (uint32_t j = 0; j < 256u; j++) {
                        const uint32_t g = S->hf[j];
                        r += g && ((g < f) || (g == f && j < i));
                    }
                    S->hw[r] = f;
                    S->horder[r] = (uint16_t)i;
                }
            }
            if (lane < 4) S->tmp[lane] = 0u;
        }
        MZ_WAVE_SYNC();
        for (uint32_t m = 0; m + 1u < nz; m++) { /* the two lightest nodes; a leaf before an inner node of the same weight */
            uint32_t w = 0;
            for (int k = 0; k < 2; k++) {
                const uint32_t lw = a < nz ? MZ_UNIFORM(S->hw[a < nz ? a : 0u]) : 0xFFFFFFFFu;
                const uint32_t iw = b < m ? MZ_UNIFORM(S->hiw[b < m ? b : 0u]) : 0xFFFFFFFFu;
                if (a < nz && (b >= m || lw <= iw)) {
                    S->hparent[a] = (uint16_t)(nz + m);
                    w += lw;
                    a++;
                } else {
                    S->hparent[nz + b] = (uint16_t)(nz + m);
                    w += iw;
                    b++;
                }
            }
            S->hiw[m] = w;
        }
        MZ_WAVE_SYNC();
        MZ_LANES {
            uint32_t deep = 0;
            for (uint32_t r = (uint32_t)lane; r < nz; r += 64u) {
                uint32_t d = 0, p = r;
                while (p != root) {
                    p = S->hparent[p];
                    d++;
                }
                deep = d > deep ? d : deep;
                S->hlen[S->horder[r]] = (uint8_t)d;
            }
            if (deep) MZ_LDS_ATOMIC_MAX(&S->tmp[0], deep);
        }
        MZ_WAVE_SYNC();
        maxlen = MZ_UNIFORM(S->tmp[0]);
        if (maxlen <= MZ_ZSE_HUF_MAX) break; /* (counts of 1 and 2 alone give no code longer than 9) */
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t i = (uint32_t)lane + 64u * k;
                if (S->hf[i]) S->hf[i] = 1u + S->hf[i] / 2u;
            }
        }
    }
    MZ_WAVE_SYNC();
    return maxlen;
}

/* The tree of S->hlen (longest code: maxlen) as weights in S->wts, the codes in the decoder's cell order in S->hcode, and its
 * description in S->wdesc; -> the description's bytes, 0 if there is no legal one.  *fse: it is the FSE-compressed form. */
MZ_DEV uint32_t mz_zse_huf_describe(mz_zse_lds *S, uint32_t maxlen, uint32_t *fse) {
    MZ_LANE_DECL
    uint32_t last = 0, n, direct, flen = 0;
    uint64_t b0, b1, b2, b3;
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t s = (uint32_t)lane + 64u * k, l = S->hlen[s];
            S->wts[s] = (uint8_t)(l ? maxlen + 1u - l : 0u);
        }
        if (lane < 16) S->rank[lane] = 0u;
    }
    MZ_BALLOT(b0, S->hlen[(uint32_t)lane] != 0u);
    MZ_BALLOT(b1, S->hlen[(uint32_t)lane + 64u] != 0u);
    MZ_BALLOT(b2, S->hlen[(uint32_t)lane + 128u] != 0u);
    MZ_BALLOT(b3, S->hlen[(uint32_t)lane + 192u] != 0u);
    last = b3 ? 255u - mz_clz64(b3) : b2 ? 191u - mz_clz64(b2) : b1 ? 127u - mz_clz64(b1) : 63u - mz_clz64(b0 | 1ull);
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t w = S->wts[(uint32_t)lane + 64u * k];
            if (w) MZ_LDS_ATOMIC_INC(&S->rank[w]);
        }
    }
    MZ_WAVE_SYNC();
    { /* rank[w] := the first cell of weight w: the lowest weights (longest codes) take the lowest cells */
        uint32_t start = 0;
        for (uint32_t w = 1; w <= maxlen; w++) {
            const uint32_t c = MZ_UNIFORM(S->rank[w]);
            S->rank[w] = start;
            start += c << (w - 1u);
        }
    }
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t s = (uint32_t)lane + 64u * k, w = S->wts[s];
            if (w) {
                uint32_t c = 0;
                for (uint32_t j = 0; j < s; j++) c += S->wts[j] == w;
                S->hcode[s] = (uint16_t)((S->rank[w] >> (w - 1u)) + c);
            }
        }
    }
    MZ_WAVE_SYNC();
    n = last; /* the weights written: those of the values in front of the last one that occurs */
    direct = n <= 128u ? 1u + ((n + 1u) >> 1) : 0u;
    if (n >= 2u) { /* FSE-compressed: two interleaved states, the one of the even positions read first (the weights' counts in hiw) */
        uint32_t distinct = 0, nsym = 0;
        MZ_LANES {
            if (lane < 16) S->hiw[lane] = 0u;
        }
        MZ_WAVE_SYNC();
        MZ_LANES {
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t s = (uint32_t)lane + 64u * k;
                if (s < n) MZ_LDS_ATOMIC_INC(&S->hiw[S->wts[s]]);
            }
        }
        MZ_WAVE_SYNC();
        for (uint32_t w = 0; w <= MZ_ZSE_HUF_MAX; w++)
            if (MZ_UNIFORM(S->hiw[w])) {
                distinct++;
                nsym = w + 1u;
            }
        if (distinct >= 2u) {
            const uint32_t al = n >= 48u ? 6u : 5u;
            uint32_t st[2] = {0, 0}, have[2] = {0, 0}, hs;
            mz_zse_lbits B;
            mz_zse_normalize(S->hiw, nsym, n, al, S->norm[0]);
            hs = mz_zse_ncount(S->norm[0], nsym, al, S->wdesc + 1);
            mz_zse_ctable(S, 0, S->norm[0], nsym, al);
            B.buf = S->wdesc + 1u + hs;
            B.n = 0;
            B.cnt = 0;
            B.acc = 0;
            for (uint32_t i = n; i-- > 0u;) {
                const uint32_t k = i & 1u, w = MZ_UNIFORM(S->wts[i]);
                if (!have[k]) {
                    st[k] = mz_zse_state0(S, 0, w);
                    have[k] = 1u;
                } else {
                    uint32_t nb, v;
                    st[k] = mz_zse_step(S, 0, st[k], w, &nb, &v);
                    mz_zse_lput(&B, nb, v);
                }
            }
            mz_zse_lput(&B, al, st[1] & ((1u << al) - 1u));
            mz_zse_lput(&B, al, st[0] & ((1u << al) - 1u));
            mz_zse_lput(&B, 1u, 1u);
            mz_zse_lpad(&B);
            MZ_WAVE_SYNC();
            if (hs + B.n <= 127u) flen = 1u + hs + B.n;
        }
    }
    if (flen && (!direct || flen < direct)) {
        S->wdesc[0] = (uint8_t)(flen - 1u);
        MZ_WAVE_SYNC();
        *fse = 1u;
        return flen;
    }
    *fse = 0u;
    if (!direct) return 0u;
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = (uint32_t)lane; k < (n + 1u) >> 1; k += 64u)
            S->wdesc[1u + k] = (uint8_t)((S->wts[2u * k] << 4) | (2u * k + 1u < n ? S->wts[2u * k + 1u] : 0u));
    }
    S->wdesc[0] = (uint8_t)(127u + n);
    MZ_WAVE_SYNC();
    return direct;
}

/* cnt literals at lit coded with S->hcode / S->hlen as one stream at dst (cap bytes there); -> the stream's bytes, 0: it did
 * not fit.  The stream is written from its last symbol to its first, 64 symbols per step. */
MZ_DEV uint32_t mz_zse_huf_stream(mz_zse_lds *S, const uint8_t *lit, uint32_t cnt, uint8_t *dst, uint32_t cap) {
    MZ_LANE_DECL
    mz_zse_bits W;
    mz_zse_open(&W, S, dst, cap);
    for (uint32_t hi = cnt; hi > 0u;) {
        const uint32_t take = hi < 64u ? hi : 64u;
        PV(uint32_t, cl);
        PV(uint32_t, cd);
        PV(uint32_t, incl);
        uint32_t base, np;
        if (W.wn + 26u > MZ_ZSE_WIN) mz_zse_flush(&W, S); /* 64 codes of 11 bits behind 31 pending ones: 23 words */
        MZ_LANES {
            P(cl) = 0;
            P(cd) = 0;
            if ((uint32_t)lane < take) {
                const uint32_t s = lit[hi - 1u - (uint32_t)lane];
                P(cl) = S->hlen[s];
                P(cd) = S->hcode[s];
            }
        }
        MZ_INCL_SCAN(incl, cl);
        base = 32u * W.wn + W.cnt;
        MZ_LANES {
            const uint32_t l = P(cl);
            if (l) {
                const uint32_t off = base + P(incl) - l, w = off >> 5, b = off & 31u;
                MZ_LDS_ATOMIC_OR(&S->win[w], P(cd) << b);
                if (b + l > 32u) MZ_LDS_ATOMIC_OR(&S->win[w + 1u], P(cd) >> (32u - b));
            }
        }
        np = base + MZ_READLANE(incl, 63);
        W.wn = np >> 5;
        W.cnt = np & 31u;
        MZ_WAVE_SYNC();
        hi -= take;
    }
    W.acc = W.cnt ? (uint64_t)(MZ_UNIFORM(S->win[W.wn]) & ((1u << W.cnt) - 1u)) : 0ull;
    MZ_WAVE_SYNC();
    S->win[W.wn] = 0u;
    MZ_WAVE_SYNC();
    return mz_zse_close(&W, S);
}

/* n bytes from src to dst by the lanes, four at a time */
MZ_DEV void mz_zse_copy(uint8_t *dst, const uint8_t *src, uint32_t n) {
    MZ_LANE_DECL
    MZ_LANES {
        for (uint32_t k = 4u * (uint32_t)lane; k + 4u <= n; k += 256u) mz_st4(dst + k, mz_ld4(src + k));
        if ((uint32_t)lane < (n & 3u)) dst[(n & ~3u) + (uint32_t)lane] = src[(n & ~3u) + (uint32_t)lane];
    }
}

/* the literals section of nlit literals at lit into dst (cap bytes); -> its bytes, 0: no room */
MZ_DEV uint32_t mz_zse_literals(mz_zse_lds *S, const uint8_t *lit, uint32_t nlit, uint8_t *dst, uint32_t cap) {
    MZ_LANE_DECL
    const uint32_t rawhdr = nlit < 32u ? 1u : nlit < 4096u ? 2u : 3u;
    uint32_t nz, kind = 0, body = 0, hdr = rawhdr;
    uint32_t dlen = 0, fse = 0, streams = 1, sz[4] = {0, 0, 0, 0}, seg = 0, comp = 0, sf = 0;
    PV(uint32_t, pc);
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t k = 0; k < 4u; k++) S->hist[(uint32_t)lane + 64u * k] = 0u;
    }
    MZ_WAVE_SYNC();
    MZ_LANES {
        for (uint32_t i = (uint32_t)lane; i < nlit; i += 64u) MZ_LDS_ATOMIC_INC(&S->hist[lit[i]]);
    }
    MZ_WAVE_SYNC();
    MZ_LANES {
        uint32_t c = 0;
        for (uint32_t k = 0; k < 4u; k++) c += S->hist[(uint32_t)lane + 64u * k] != 0u;
        P(pc) = c;
    }
    MZ_WAVE_SUM(nz, pc);
    if (nz == 1u) {
        kind = 1u; /* RLE */
    } else if (nz >= 2u) {
        const uint32_t maxlen = mz_zse_huf_lengths(S);
        dlen = mz_zse_huf_describe(S, maxlen, &fse);
        if (dlen) {
            PV(uint32_t, q0);
            PV(uint32_t, q1);
            PV(uint32_t, q2);
            PV(uint32_t, q3);
            uint32_t bits[4];
            streams = nlit <= 1023u ? 1u : 4u;
            seg = streams == 1u ? nlit : (nlit + 3u) >> 2;
            MZ_LANES {
                uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                for (uint32_t i = (uint32_t)lane; i < nlit; i += 64u) {
                    const uint32_t l = S->hlen[lit[i]], k = (i >= seg) + (i >= 2u * seg) + (i >= 3u * seg);
                    a0 += k == 0u ? l : 0u;
                    a1 += k == 1u ? l : 0u;
                    a2 += k == 2u ? l : 0u;
                    a3 += k >= 3u ? l : 0u;
                }
                P(q0) = a0;
                P(q1) = a1;
                P(q2) = a2;
                P(q3) = a3;
            }
            MZ_WAVE_SUM(bits[0], q0);
            MZ_WAVE_SUM(bits[1], q1);
            MZ_WAVE_SUM(bits[2], q2);
            MZ_WAVE_SUM(bits[3], q3);
            comp = dlen + (streams == 4u ? 6u : 0u);
            for (uint32_t k = 0; k < streams; k++) {
                sz[k] = bits[k] / 8u + 1u;
                comp += sz[k];
            }
            sf = streams == 1u ? 0u : (nlit < 16384u && comp < 16384u) ? 2u : 3u;
            hdr = sf < 2u ? 3u : sf + 2u;
            if (hdr + comp < rawhdr + nlit && sz[0] < 65536u && sz[1] < 65536u && sz[2] < 65536u) kind = 2u;
        }
    }
    if (kind == 2u) {
        const uint32_t nb = sf < 2u ? 10u : sf == 2u ? 14u : 18u;
        const uint64_t h = 2ull | ((uint64_t)sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)comp << (4u + nb));
        uint32_t p = hdr, d0 = 0;
        if (hdr + comp > cap) return 0u;
        for (uint32_t k = 0; k < hdr; k++) dst[k] = (uint8_t)(h >> (8u * k));
        MZ_LANES {
            for (uint32_t k = (uint32_t)lane; k < dlen; k += 64u) dst[p + k] = S->wdesc[k];
        }
        p += dlen;
        if (streams == 4u) {
            for (uint32_t k = 0; k < 3u; k++) {
                dst[p + 2u * k] = (uint8_t)sz[k];
                dst[p + 2u * k + 1u] = (uint8_t)(sz[k] >> 8);
            }
            p += 6u;
        }
        for (uint32_t k = 0; k < streams; k++) {
            const uint32_t dn = (streams == 4u && k < 3u) ? seg : nlit - d0;
            const uint32_t got = mz_zse_huf_stream(S, lit + d0, dn, dst + p, sz[k]);
            if (got != sz[k]) return 0u; /* (cannot happen: the sizes are sums of the same lengths) */
            p += got;
            d0 += dn;
        }
        return p;
    }
    body = kind == 1u ? 1u : nlit;
    if (rawhdr + body > cap) return 0u;
    {
        const uint32_t h = rawhdr == 1u ? (kind | (nlit << 3)) : (kind | ((rawhdr == 2u ? 1u : 3u) << 2) | (nlit << 4));
        for (uint32_t k = 0; k < rawhdr; k++) dst[k] = (uint8_t)(h >> (8u * k));
    }
    if (kind == 1u) {
        dst[rawhdr] = (uint8_t)MZ_UNIFORM((uint32_t)lit[0]);
    } else {
        mz_zse_copy(dst + rawhdr, lit, nlit);
    }
    return rawhdr + body;
}

/* flags: bit 0 = write the XXH64 content checksum.  tok / ntok: the entry's token blocks (block b at tok + b * MZ_DEF_BLOCK,
 * ntok[b] of them).  scratch: MZ_ZSE_SCRATCH_BYTES of this wave.  All arguments wave-uniform. */
MZ_DEV void mz_zstd_enc_entry(const uint8_t *in, uint32_t in_len, const uint32_t *tok, const uint32_t *ntok, uint8_t *out, uint32_t out_cap,
                              uint32_t flags, mz_zse_lds *S, const uint32_t *crc_tab, const mzhip_crc_tables *tabs, uint8_t *scratch,
                              mz_zse_result *res) {
    MZ_LANE_DECL
    uint8_t *const lit = scratch;
    uint32_t *const seqA = (uint32_t *)(scratch + MZ_DEF_BLOCK); /* literal length | (match length - 3) << 16 */
    uint32_t *const seqB = seqA + MZ_ZSE_MAXSEQ;                 /* the distance, then the offset value */
    uint8_t *const stage = (uint8_t *)(seqB + MZ_ZSE_MAXSEQ);
    const uint32_t nblocks = in_len ? (in_len + MZ_DEF_BLOCK - 1u) / MZ_DEF_BLOCK : 1u;
    uint32_t o = 0, fail = 0, rep0 = 1, rep1 = 4, rep2 = 8, crc = 0;
    MZ_ZSEPROF_INIT

#define MZ_ZSE_OUT(nbytes, val)                                                                              \
    do {                                                                                                     \
        const uint32_t _n = (nbytes), _v = (val);                                                            \
        if (_n > out_cap - o) fail = 1u;                                                                     \
        if (!fail) {                                                                                         \
            for (uint32_t _k = 0; _k < _n; _k++) out[o + _k] = (uint8_t)(_v >> (8u * _k)); /* wave-uniform */ \
            o += _n;                                                                                         \
        }                                                                                                    \
    } while (0)

    /* ---- the frame header */
    MZ_ZSE_OUT(4u, 0xFD2FB528u);
    if (in_len <= MZ_LZE_FAR_DICT) {
        const uint32_t f = in_len < 256u ? 0u : in_len < 65792u ? 1u : 2u;
        MZ_ZSE_OUT(1u, (f << 6) | 0x20u | ((flags & 1u) << 2));
        MZ_ZSE_OUT(f == 0u ? 1u : f == 1u ? 2u : 4u, f == 1u ? in_len - 256u : in_len);
    } else {
        MZ_ZSE_OUT(1u, 0x80u | ((flags & 1u) << 2));
        MZ_ZSE_OUT(1u, (23u - 10u) << 3); /* a window of 8 MiB: every distance is below MZ_LZE_FAR_DICT */
        MZ_ZSE_OUT(4u, in_len);
    }

    for (uint32_t b = 0; b < nblocks && !fail; b++) {
        const uint32_t bs = b * MZ_DEF_BLOCK, blen = in_len - bs < MZ_DEF_BLOCK ? in_len - bs : MZ_DEF_BLOCK, lastb = b + 1u == nblocks ? 1u : 0u;
        const uint8_t *const src = in + bs;
        const uint32_t *const bt = tok + (size_t)b * MZ_DEF_BLOCK;
        const uint32_t nt_blk = in_len ? MZ_UNIFORM(ntok[b]) : 0u;
        const uint32_t r0 = rep0, r1 = rep1, r2 = rep2;
        uint32_t nlit = 0, nseq = 0, csize = 0, equal = blen ? 1u : 0u;

        /* ---- are the block's bytes all equal?  (stops at the first step that sees a difference) */
        if (blen) {
            const uint32_t first = MZ_UNIFORM((uint32_t)src[0]);
            for (uint32_t p = 0; p < blen && equal; p += 512u) {
                uint64_t diff;
                PV(uint32_t, df);
                MZ_LANES {
                    const uint32_t q = p + 8u * (uint32_t)lane;
                    uint32_t d = 0;
                    if (q + 8u <= blen) {
                        d = mz_ld8(src + q) != 0x0101010101010101ull * first;
                    } else {
                        for (uint32_t k = 0; k < 8u; k++)
                            if (q + k < blen) d |= src[q + k] != first;
                    }
                    P(df) = d;
                }
                MZ_BALLOT(diff, P(df) != 0u);
                if (diff) equal = 0u;
            }
        }
        if (equal) {
            MZ_ZSE_OUT(3u, (blen << 3) | 2u | lastb);
            MZ_ZSE_OUT(1u, MZ_UNIFORM((uint32_t)src[0]));
            continue;
        }

        /* ---- 1. tokens -> literals and sequences */
        {
            uint32_t pv = 0, p_ll = 0, p_ml = 0, p_dist = 0, carry_ll = 0, prev_tok = 0;
            for (uint32_t t0 = 0; t0 < nt_blk; t0 += 64u) {
                const uint32_t nt = nt_blk - t0 < 64u ? nt_blk - t0 : 64u;
                PV(uint32_t, tk);
                PV(uint32_t, mlen);
                PV(uint32_t, isl);
                PV(uint32_t, tprev);
                PV(uint32_t, cont);
                PV(uint32_t, st);
                PV(uint32_t, li);
                PV(uint32_t, mi);
                PV(uint32_t, me);
                PV(uint32_t, eidx);
                PV(uint32_t, llv);
                PV(uint32_t, mlv);
                uint64_t mm, cm, sm;
                uint32_t lead, ns;
                MZ_LANES {
                    const uint32_t t = ((uint32_t)lane < nt) ? bt[t0 + (uint32_t)lane] : 0u;
                    P(tk) = t;
                    P(mlen) = t & 511u;
                    P(isl) = ((uint32_t)lane < nt && (t & 511u) == 0u) ? 1u : 0u;
                }
                MZ_GATHER4(tprev, tk, 4u * (((uint32_t)lane - 1u) & 63u));
                MZ_LANES {
                    const uint32_t pt = lane == 0 ? prev_tok : P(tprev);
                    P(cont) = (P(mlen) && (pt & 511u) && (pt >> 9) == (P(tk) >> 9)) ? 1u : 0u;
                    P(st) = (P(mlen) && !P(cont)) ? 1u : 0u;
                }
                MZ_INCL_SCAN(li, isl);
                MZ_INCL_SCAN(mi, mlen);
                MZ_BALLOT(mm, P(mlen) != 0u);
                MZ_BALLOT(cm, P(cont) != 0u);
                MZ_BALLOT(sm, P(st) != 0u);
                MZ_LANES {
                    if (P(isl)) lit[nlit + P(li) - 1u] = (uint8_t)(P(tk) >> 9); /* < blen: a literal is a byte of the block */
                    { /* where this lane's run of matches ends */
                        const uint64_t nc = ~cm & ~(((uint64_t)2 << lane) - 1ull);
                        P(eidx) = nc ? mz_ctz64(nc) - 1u : 63u;
                    }
                }
                MZ_GATHER(me, mi, P(eidx));
                lead = ~cm ? mz_ctz64(~cm) : 64u; /* the matches in front that go on the open sequence */
                if (lead) p_ml += MZ_READLANE(mi, lead - 1u);
                ns = mz_popc64(sm);
                MZ_LANES {
                    const uint64_t below = mm & (((uint64_t)1 << lane) - 1ull);
                    P(llv) = below ? (uint32_t)lane - 1u - (63u - mz_clz64(below)) : (uint32_t)lane + carry_ll;
                    P(mlv) = P(me) - P(mi) + P(mlen);
                    if (P(st)) {
                        const uint32_t r = MZ_RANK_BELOW(sm);
                        if (r + 1u < ns) {
                            const uint32_t idx = nseq + pv + r; /* < MZ_ZSE_MAXSEQ: every sequence holds a match of 4 bytes */
                            seqA[idx] = P(llv) | ((P(mlv) - 3u) << 16);
                            seqB[idx] = P(tk) >> 9;
                        }
                    }
                }
                if (ns) {
                    const uint32_t ls = 63u - mz_clz64(sm);
                    if (pv) {
                        seqA[nseq] = p_ll | ((p_ml - 3u) << 16); /* wave-uniform stores */
                        seqB[nseq] = p_dist;
                    }
                    nseq += pv + ns - 1u;
                    pv = 1u;
                    p_ll = MZ_READLANE(llv, ls);
                    p_ml = MZ_READLANE(mlv, ls);
                    p_dist = MZ_READLANE(tk, ls) >> 9;
                }
                carry_ll = mm ? nt - 1u - (63u - mz_clz64(mm)) : carry_ll + nt;
                nlit += MZ_READLANE(li, 63);
                prev_tok = MZ_READLANE(tk, nt - 1u);
            }
            if (pv) {
                seqA[nseq] = p_ll | ((p_ml - 3u) << 16);
                seqB[nseq] = p_dist;
                nseq++;
            }
        }
        MZ_ZSE_NOTE_NSEQ(nseq);
        MZ_CHASE_FENCE(); /* literals and records were stored a lane each and are read through other lanes from here on */
        MZ_WAVE_SYNC();

        /* ---- 2. repeat offsets in stream order; the codes' histograms */
        MZ_LANES {
            for (uint32_t k = 0; k < 3u; k++) S->shist[k][lane] = 0u;
        }
        MZ_WAVE_SYNC();
        for (uint32_t s0 = 0; s0 < nseq; s0 += 64u) {
            const uint32_t cnt = nseq - s0 < 64u ? nseq - s0 : 64u;
            PV(uint32_t, ra);
            PV(uint32_t, rb);
            PV(uint32_t, ov);
            MZ_LANES {
                P(ra) = (uint32_t)lane < cnt ? seqA[s0 + (uint32_t)lane] : 0u;
                P(rb) = (uint32_t)lane < cnt ? seqB[s0 + (uint32_t)lane] : 0u;
                P(ov) = 0u;
            }
            for (uint32_t i = 0; i < cnt; i++) {
                const uint32_t ll = MZ_READLANE(ra, i) & 0xFFFFu, d = MZ_READLANE(rb, i);
                uint32_t v;
                if (ll) {
                    if (d == rep0) {
                        v = 1u;
                    } else if (d == rep1) {
                        v = 2u;
                        rep1 = rep0;
                        rep0 = d;
                    } else {
                        v = d == rep2 ? 3u : d + 3u;
                        rep2 = rep1;
                        rep1 = rep0;
                        rep0 = d;
                    }
                } else {
                    if (d == rep1) {
                        v = 1u;
                        rep1 = rep0;
                        rep0 = d;
                    } else {
                        v = d == rep2 ? 2u : d == rep0 - 1u ? 3u : d + 3u; /* (d >= 1: rep0 - 1 == 0 names nothing) */
                        rep2 = rep1;
                        rep1 = rep0;
                        rep0 = d;
                    }
                }
                MZ_WRITELANE(ov, i, v);
            }
            MZ_LANES {
                if ((uint32_t)lane < cnt) {
                    seqB[s0 + (uint32_t)lane] = P(ov);
                    MZ_LDS_ATOMIC_INC(&S->shist[0][mz_zse_ll_code(P(ra) & 0xFFFFu)]);
                    MZ_LDS_ATOMIC_INC(&S->shist[1][mz_zs_highbit(P(ov))]);
                    MZ_LDS_ATOMIC_INC(&S->shist[2][mz_zse_ml_code(P(ra) >> 16)]);
                }
            }
        }
        MZ_CHASE_FENCE();
        MZ_WAVE_SYNC();
        MZ_ZSEPROF_MARK(0);

        /* ---- 3. the literals section */
        csize = mz_zse_literals(S, lit, nlit, stage, MZ_ZSE_STAGE_BYTES);
        MZ_ZSEPROF_MARK(2);

        /* ---- 4. the sequences section */
        if (csize && nseq == 0u) {
            stage[csize] = 0u; /* wave-uniform store */
            csize += 1u;
        } else if (csize) {
            uint32_t mode[3], al[3], dl[3], p = csize;
            for (uint32_t t = 0; t < 3u; t++) {
                const uint32_t max_al = t == 1u ? 8u : 9u, def_al = t == 1u ? 5u : 6u, def_n = t == 0u ? 36u : t == 1u ? 29u : 53u;
                uint32_t present = 0, nsym = 0, only = 0;
                uint64_t pm;
                MZ_BALLOT(pm, S->shist[t][lane] != 0u);
                present = mz_popc64(pm);
                nsym = 64u - mz_clz64(pm); /* (a block with a sequence: pm != 0) */
                only = mz_ctz64(pm);
                if (present == 1u) {
                    mode[t] = 1u;
                    al[t] = 0u;
                    dl[t] = 1u;
                    MZ_WAVE_SYNC();
                    S->desc[t][0] = (uint8_t)only;
                    S->dnb[t][only] = 0u;
                    S->dfs[t][only] = 0;
                    S->stt[t][0] = 0u;
                    MZ_WAVE_SYNC();
                } else {
                    uint32_t a = mz_zs_highbit(nseq - 1u) > 2u ? mz_zs_highbit(nseq - 1u) - 2u : 0u, cf, cp;
                    a = a < 5u ? 5u : a > max_al ? max_al : a;
                    while ((1u << a) < 2u * present) a++; /* (53 codes at the most: 7) */
                    mz_zse_normalize(S->shist[t], nsym, nseq, a, S->norm[t]);
                    dl[t] = mz_zse_ncount(S->norm[t], nsym, a, S->desc[t]);
                    cf = mz_zse_cost(S->shist[t], S->norm[t], nsym, a) + (dl[t] << 11);
                    MZ_LANES {
                        if ((uint32_t)lane < def_n) S->dnorm[lane] = t == 0u ? mz_zs_dll[lane < 36 ? lane : 0] : t == 1u ? mz_zs_dof[lane < 29 ? lane : 0] : mz_zs_dml[lane < 53 ? lane : 0];
                    }
                    MZ_WAVE_SYNC();
                    cp = nsym <= def_n ? mz_zse_cost(S->shist[t], S->dnorm, nsym, def_al) : 0xFFFFFFFFu;
                    if (cp <= cf) {
                        mode[t] = 0u;
                        al[t] = def_al;
                        dl[t] = 0u;
                        mz_zse_ctable(S, t, S->dnorm, def_n, def_al);
                    } else {
                        mode[t] = 2u;
                        al[t] = a;
                        mz_zse_ctable(S, t, S->norm[t], nsym, a);
                    }
                }
            }
            MZ_ZSEPROF_MARK(1);
            if (p + 3u + dl[0] + dl[1] + dl[2] > MZ_ZSE_STAGE_BYTES) {
                csize = 0u;
            } else {
                mz_zse_bits W;
                uint32_t sl = 0, so = 0, sm2 = 0, first = 1u;
                if (nseq < 128u) {
                    stage[p++] = (uint8_t)nseq;
                } else {
                    stage[p++] = (uint8_t)(128u + (nseq >> 8));
                    stage[p++] = (uint8_t)nseq;
                }
                stage[p++] = (uint8_t)((mode[0] << 6) | (mode[1] << 4) | (mode[2] << 2));
                for (uint32_t t = 0; t < 3u; t++) {
                    const uint32_t n = dl[t];
                    uint8_t *const q = stage + p;
                    MZ_LANES {
                        for (uint32_t k = (uint32_t)lane; k < n; k += 64u) q[k] = S->desc[t][k];
                    }
                    p += n;
                }
                mz_zse_open(&W, S, stage + p, MZ_ZSE_STAGE_BYTES - p);
                for (uint32_t hi = nseq; hi > 0u && !W.fail;) {
                    const uint32_t cnt = hi < 64u ? hi : 64u, base = hi - cnt;
                    PV(uint32_t, cds);
                    PV(uint32_t, xa);
                    PV(uint32_t, xb);
                    MZ_LANES {
                        uint32_t c = 0, x = 0, y = 0;
                        if ((uint32_t)lane < cnt) {
                            const uint32_t A = seqA[base + (uint32_t)lane], ov = seqB[base + (uint32_t)lane];
                            const uint32_t ll = A & 0xFFFFu, mlb = A >> 16;
                            const uint32_t lc = mz_zse_ll_code(ll), mc = mz_zse_ml_code(mlb), oc = mz_zs_highbit(ov);
                            uint32_t nb;
                            c = lc | (mc << 8) | (oc << 16);
                            x = (ll - mz_zs_ll_base(lc, &nb)) | ((mlb + 3u - mz_zs_ml_base(mc, &nb)) << 16);
                            y = ov - (1u << oc);
                        }
                        P(cds) = c;
                        P(xa) = x;
                        P(xb) = y;
                    }
                    for (uint32_t i = cnt; i-- > 0u;) {
                        const uint32_t c = MZ_READLANE(cds, i), x = MZ_READLANE(xa, i), y = MZ_READLANE(xb, i);
                        const uint32_t lc = c & 255u, mc = (c >> 8) & 255u, oc = c >> 16;
                        uint32_t nbl, nbm, dummy;
                        if (first) {
                            sl = mz_zse_state0(S, 0, lc);
                            so = mz_zse_state0(S, 1, oc);
                            sm2 = mz_zse_state0(S, 2, mc);
                            first = 0u;
                        } else {
                            uint32_t nb, v;
                            so = mz_zse_step(S, 1, so, oc, &nb, &v);
                            mz_zse_put(&W, S, nb, v);
                            sm2 = mz_zse_step(S, 2, sm2, mc, &nb, &v);
                            mz_zse_put(&W, S, nb, v);
                            sl = mz_zse_step(S, 0, sl, lc, &nb, &v);
                            mz_zse_put(&W, S, nb, v);
                        }
                        dummy = mz_zs_ll_base(lc, &nbl);
                        dummy = mz_zs_ml_base(mc, &nbm);
                        (void)dummy;
                        mz_zse_put(&W, S, nbl, x & 0xFFFFu);
                        mz_zse_put(&W, S, nbm, x >> 16);
                        mz_zse_put(&W, S, oc, y);
                    }
                    hi = base;
                }
                mz_zse_put(&W, S, al[2], sm2 & ((1u << al[2]) - 1u));
                mz_zse_put(&W, S, al[1], so & ((1u << al[1]) - 1u));
                mz_zse_put(&W, S, al[0], sl & ((1u << al[0]) - 1u));
                {
                    const uint32_t got = mz_zse_close(&W, S);
                    csize = got ? p + got : 0u;
                }
            }
        }
        MZ_CHASE_FENCE(); /* the staged body was stored through some lanes' addresses and is copied through others' */
        MZ_WAVE_SYNC();
        MZ_ZSEPROF_MARK(3);

        /* ---- 5. the block */
        if (csize && csize < blen) {
            MZ_ZSE_OUT(3u, (csize << 3) | 4u | lastb);
            if (csize > out_cap - o) fail = 1u;
            if (!fail) {
                mz_zse_copy(out + o, stage, csize);
                o += csize;
            }
        } else {
            rep0 = r0; /* a Raw block leaves the repeat offsets alone */
            rep1 = r1;
            rep2 = r2;
            MZ_ZSE_OUT(3u, (blen << 3) | lastb);
            if (blen > out_cap - o) fail = 1u;
            if (!fail) {
                mz_zse_copy(out + o, src, blen);
                o += blen;
            }
        }
        MZ_ZSEPROF_MARK(4);
    }
    if ((flags & 1u) && !fail) {
        const uint32_t x = mz_zs_xxh64(in, in_len);
        MZ_ZSE_OUT(4u, x);
    }
#undef MZ_ZSE_OUT

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
    MZ_ZSEPROF_MARK(4);
    MZ_ZSEPROF_FLUSH
    res->out_len = fail ? 0u : o;
    res->crc = crc;
    res->status = fail ? MZHIP_OUT_FULL : MZHIP_OK;
}

#endif
