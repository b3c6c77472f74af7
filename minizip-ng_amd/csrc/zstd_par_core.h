/* zstd_par_core.h -- ONE large Zstandard entry decoded by a wave per block: the device passes behind mzhip_zstd_large
 * (the host logic between them: zstd_parallel.inc).
 *
 * Written in the wave.h vocabulary like zstd_core.h, whose readers (input window, FSE and Huffman tables, literals) it
 * uses unchanged: the same text is the gfx950 kernel bodies (k_zstd_scan, k_zstd_blocks, k_zstd_frame_xxh) and, under
 * g++ -DMZHIP_HOST_EMUL, the host build of the CPU tests (tests/emul/emul_zstd_large.cpp).
 *
 * A block's end stands in its 3-byte header, so nothing is searched.  What a block needs from the blocks before it is
 *   - the Huffman tree of treeless literals and a sequence table in Repeat_Mode: both are DESCRIPTIONS in an earlier
 *     block's bytes; the host names that block (the "definer") and the wave builds the table from there;
 *   - the three repeat offsets: the count pass reports a block's offsets behind it as a function of those in front of
 *     it, the host composes the functions along the frame;
 *   - the bytes matches copy: the emit pass writes, per match byte, the INDEX of its source (a source map); pointer
 *     jumping resolves the map (k_ptr_jump / k_ptr_gather, shared with the DEFLATE path).
 *
 *   scan    one wave: frame and block headers of the whole entry, a record per block and per frame;
 *   count   a wave per Compressed block: the three tables, the FSE machine without executing anything -> bytes produced,
 *           the repeat-offset function;
 *   emit    a wave per block: literals decoded, sequences decoded, literal bytes to out[] with ptr[i] = i, match bytes
 *           as ptr[m0 + k] = m0 - dist + (dist < ml ? k % dist : k).  No earlier output is read.
 * Every pass reports a problem instead of a status: the caller then decodes the whole entry with mz_zstd_entry, which
 * is what keeps statuses, lengths and bytes those of the one-wave reader.
 */
#ifndef MZHIP_ZSTD_PAR_CORE_H
#define MZHIP_ZSTD_PAR_CORE_H

#include "zstd_core.h"

#define MZ_ZSP_BLOCK_CAP 32768u /* block records per entry: 4 GiB of 128 KiB blocks */
#define MZ_ZSP_REC_WORDS 16u
#define MZ_ZSP_FRM_WORDS 8u
#define MZ_ZSP_JOB_WORDS 32u
#define MZ_ZSP_RES_WORDS 8u
#define MZ_ZSP_HDR_WORDS 8u

/* a block record of the scan */
enum {
    MZ_ZSP_R_OFF = 0,  /* the block header's offset in the input */
    MZ_ZSP_R_SIZE,     /* Block_Size */
    MZ_ZSP_R_TYPE,     /* Block_Type | Last_Block << 2 */
    MZ_ZSP_R_FRAME,    /* index of its frame record */
    MZ_ZSP_R_LIT,      /* Compressed blocks: Literals_Block_Type | Size_Format << 2 */
    MZ_ZSP_R_REGEN,    /* Regenerated_Size */
    MZ_ZSP_R_COMP,     /* Compressed_Size (Compressed and Treeless literals) */
    MZ_ZSP_R_TREE,     /* where the Huffman tree description starts (Compressed literals) */
    MZ_ZSP_R_SEQ,      /* where the sequences section starts */
    MZ_ZSP_R_NSEQ,     /* Number_of_Sequences */
    MZ_ZSP_R_MODES,    /* the modes byte (nseq > 0) */
    MZ_ZSP_R_TABS      /* where the table descriptions start (nseq > 0) */
};
/* a frame record */
enum {
    MZ_ZSP_F_BLKMAX = 0, /* min(Window_Size, 128 KiB) */
    MZ_ZSP_F_FCS_LO,
    MZ_ZSP_F_FCS_HI,
    MZ_ZSP_F_FLAGS,      /* 1 Frame_Content_Size present, 2 Content_Checksum present */
    MZ_ZSP_F_END,        /* the offset behind the frame (its checksum included) */
    MZ_ZSP_F_CHECK       /* the stored checksum */
};
/* the header the scan leaves */
enum {
    MZ_ZSP_H_NBLK = 0,
    MZ_ZSP_H_NFRM,
    MZ_ZSP_H_STOP, /* 0 the end of the input, 1 the block cap, 2 a problem */
    MZ_ZSP_H_AT    /* where it stopped */
};
/* a job of the count and emit passes: the block, and what the host knows about its surroundings */
enum {
    MZ_ZSP_J_OFF = 0,
    MZ_ZSP_J_SIZE,
    MZ_ZSP_J_TYPE,
    MZ_ZSP_J_BLKMAX,
    MZ_ZSP_J_REGEN,
    MZ_ZSP_J_SEQ,
    MZ_ZSP_J_POS,      /* emit: the block's first output byte */
    MZ_ZSP_J_END,      /* emit: the byte behind its last (from the count pass) */
    MZ_ZSP_J_FO,       /* emit: the frame's first output byte */
    MZ_ZSP_J_REP0,     /* emit: the repeat offsets in front of the block (three words) */
    MZ_ZSP_J_TREE = 12, /* treeless literals: the definer's tree description [TREE, TREE_END) */
    MZ_ZSP_J_TREE_END,
    MZ_ZSP_J_DEF = 14  /* per table LL / OF / ML three words: the definer's first table byte, its modes byte, its block's end
                        * (all 0: the table is described in this block) */
};
/* a result: status (0, or 1 for any problem), bytes produced, and per outgoing repeat-offset slot (source, value):
 * source 3 = the distance `value`; source j < 3 = incoming slot j minus `value` */
enum { MZ_ZSP_O_STATUS = 0, MZ_ZSP_O_BYTES, MZ_ZSP_O_REP = 2 };

#define MZ_ZSP_STOP(code, at)                      \
    do {                                           \
        hdr[MZ_ZSP_H_STOP] = (code);               \
        hdr[MZ_ZSP_H_AT] = (at);                   \
        goto out;                                  \
    } while (0)

/* ---- scan: the headers of the whole entry on one wave.  Wave-uniform values are stored by all lanes. */
MZ_DEV void mz_zsp_scan(const uint8_t *in, uint32_t in_len, mz_zs_lds *S, uint32_t *recs, uint32_t *frms, uint32_t blk_cap, uint32_t *hdr) {
    mz_zs_ctx ctx;
    mz_zs_ctx *const C = &ctx;
    uint32_t p = 0, nblk = 0, nfrm = 0, magic = 0, fhd = 0, single = 0, n = 0, wd = 0, last = 0, bh = 0, type = 0, bs = 0, blk_max = 0;
    uint64_t wsize = 0, fcs = 0;
    C->in = in;
    C->in_len = in_len;
    C->base = 0u - MZ_ZS_INBUF;
    if (in_len == 0) MZ_ZSP_STOP(2u, 0u);
    while (p < in_len) {
        if (in_len - p < 4u) MZ_ZSP_STOP(2u, p);
        magic = mz_zs_le(C, S, p, 4);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            if (in_len - p < 8u) MZ_ZSP_STOP(2u, p);
            n = mz_zs_le(C, S, p + 4u, 4);
            if (n > in_len - p - 8u) MZ_ZSP_STOP(2u, p);
            p += 8u + n;
            continue;
        }
        if (magic != 0xFD2FB528u) MZ_ZSP_STOP(2u, p);
        p += 4u;
        if (p >= in_len) MZ_ZSP_STOP(2u, p);
        fhd = mz_zs_byte(C, S, p);
        p += 1u;
        if (fhd & 8u) MZ_ZSP_STOP(2u, p);
        single = (fhd >> 5) & 1u;
        wsize = 0;
        if (!single) {
            if (p >= in_len) MZ_ZSP_STOP(2u, p);
            wd = mz_zs_byte(C, S, p);
            p += 1u;
            if (10u + (wd >> 3) > 31u) MZ_ZSP_STOP(2u, p);
            wsize = 1ull << (10u + (wd >> 3));
            wsize += (wsize >> 3) * (wd & 7u);
        }
        n = (fhd & 3u) == 3u ? 4u : (fhd & 3u);
        if (n > in_len - p) MZ_ZSP_STOP(2u, p);
        if (mz_zs_le(C, S, p, n) != 0) MZ_ZSP_STOP(2u, p);
        p += n;
        n = (fhd >> 6) ? (1u << (fhd >> 6)) : single;
        if (n > in_len - p) MZ_ZSP_STOP(2u, p);
        fcs = mz_zs_le(C, S, p, n < 4u ? n : 4u);
        if (n == 8u) fcs |= (uint64_t)mz_zs_le(C, S, p + 4u, 4) << 32;
        if (n == 2u) fcs += 256u;
        p += n;
        if (single) wsize = fcs;
        blk_max = wsize < MZ_ZS_BLOCK_MAX ? (uint32_t)wsize : MZ_ZS_BLOCK_MAX;
        {
            uint32_t *f = frms + (size_t)nfrm * MZ_ZSP_FRM_WORDS;
            f[MZ_ZSP_F_BLKMAX] = blk_max;
            f[MZ_ZSP_F_FCS_LO] = (uint32_t)fcs;
            f[MZ_ZSP_F_FCS_HI] = (uint32_t)(fcs >> 32);
            f[MZ_ZSP_F_FLAGS] = (n != 0 ? 1u : 0u) | ((fhd & 4u) ? 2u : 0u);
            f[MZ_ZSP_F_END] = 0;
            f[MZ_ZSP_F_CHECK] = 0;
            f[6] = 0;
            f[7] = 0;
        }
        do {
            uint32_t *r;
            if (nblk >= blk_cap) MZ_ZSP_STOP(1u, p);
            if (in_len - p < 3u) MZ_ZSP_STOP(2u, p);
            bh = mz_zs_le(C, S, p, 3);
            last = bh & 1u;
            type = (bh >> 1) & 3u;
            bs = bh >> 3;
            if (type == 3u || bs > blk_max) MZ_ZSP_STOP(2u, p);
            r = recs + (size_t)nblk * MZ_ZSP_REC_WORDS;
            for (uint32_t k = 0; k < MZ_ZSP_REC_WORDS; k++) r[k] = 0;
            r[MZ_ZSP_R_OFF] = p;
            r[MZ_ZSP_R_SIZE] = bs;
            r[MZ_ZSP_R_TYPE] = type | (last << 2);
            r[MZ_ZSP_R_FRAME] = nfrm;
            if (type == 0) {
                if (bs > in_len - p - 3u) MZ_ZSP_STOP(2u, p);
                p += 3u + bs;
            } else if (type == 1u) {
                if (p + 3u >= in_len) MZ_ZSP_STOP(2u, p);
                p += 4u;
            } else {
                const uint32_t q = p + 3u, end = q + bs;
                uint32_t b0, lt, sf, hl, regen, comp = 0, sp, nseq;
                if (bs > in_len - q || bs < 3u || bs >= MZ_ZS_BLOCK_MAX) MZ_ZSP_STOP(2u, p);
                b0 = mz_zs_byte(C, S, q);
                lt = b0 & 3u;
                sf = (b0 >> 2) & 3u;
                if (lt < 2u) {
                    hl = (sf & 1u) ? (sf == 1u ? 2u : 3u) : 1u;
                    regen = (sf & 1u) ? (mz_zs_le(C, S, q, hl) >> 4) : (b0 >> 3);
                    if (regen > blk_max) MZ_ZSP_STOP(2u, p);
                    if (lt == 0) {
                        if (regen > bs - hl) MZ_ZSP_STOP(2u, p);
                        sp = q + hl + regen;
                    } else {
                        sp = q + hl + 1u;
                    }
                } else {
                    hl = sf < 2u ? 3u : sf + 2u;
                    if (hl > bs) MZ_ZSP_STOP(2u, p);
                    if (sf < 2u) {
                        const uint32_t v = mz_zs_le(C, S, q, 3) >> 4;
                        regen = v & 1023u;
                        comp = v >> 10;
                    } else if (sf == 2u) {
                        const uint32_t v = mz_zs_le(C, S, q, 4) >> 4;
                        regen = v & 16383u;
                        comp = v >> 14;
                    } else {
                        const uint32_t v = mz_zs_le(C, S, q, 4) >> 4;
                        regen = v & 262143u;
                        comp = (v >> 18) | (mz_zs_byte(C, S, q + 4u) << 10);
                    }
                    if (regen == 0 || regen > blk_max || comp > bs - hl) MZ_ZSP_STOP(2u, p);
                    sp = q + hl + comp;
                    r[MZ_ZSP_R_TREE] = q + hl;
                }
                if (sp >= end) MZ_ZSP_STOP(2u, p);
                b0 = mz_zs_byte(C, S, sp);
                if (b0 < 128u) {
                    nseq = b0;
                    n = 1u;
                } else if (b0 < 255u) {
                    if (end - sp < 2u) MZ_ZSP_STOP(2u, p);
                    nseq = ((b0 - 128u) << 8) + mz_zs_byte(C, S, sp + 1u);
                    n = 2u;
                } else {
                    if (end - sp < 3u) MZ_ZSP_STOP(2u, p);
                    nseq = mz_zs_le(C, S, sp + 1u, 2) + 0x7F00u;
                    n = 3u;
                }
                if (nseq) {
                    if (sp + n >= end) MZ_ZSP_STOP(2u, p);
                    const uint32_t modes = mz_zs_byte(C, S, sp + n);
                    if (modes & 3u) MZ_ZSP_STOP(2u, p);
                    r[MZ_ZSP_R_MODES] = modes;
                    r[MZ_ZSP_R_TABS] = sp + n + 1u;
                } else if (sp + n != end) {
                    MZ_ZSP_STOP(2u, p);
                }
                r[MZ_ZSP_R_LIT] = lt | (sf << 2);
                r[MZ_ZSP_R_REGEN] = regen;
                r[MZ_ZSP_R_COMP] = comp;
                r[MZ_ZSP_R_SEQ] = sp;
                r[MZ_ZSP_R_NSEQ] = nseq;
                p = end;
            }
            nblk++;
        } while (!last);
        {
            uint32_t *f = frms + (size_t)nfrm * MZ_ZSP_FRM_WORDS;
            if (fhd & 4u) {
                if (in_len - p < 4u) MZ_ZSP_STOP(2u, p);
                f[MZ_ZSP_F_CHECK] = mz_zs_le(C, S, p, 4);
                p += 4u;
            }
            f[MZ_ZSP_F_END] = p;
        }
        nfrm++;
    }
    hdr[MZ_ZSP_H_STOP] = 0;
    hdr[MZ_ZSP_H_AT] = p;
out:
    hdr[MZ_ZSP_H_NBLK] = nblk;
    hdr[MZ_ZSP_H_NFRM] = nfrm;
}

#if defined(MZHIP_HOST_EMUL)
#define MZ_ZSP_UNROLL
#else
#define MZ_ZSP_UNROLL _Pragma("unroll")
#endif

/* the low 32 bits of XXH64(d[0 .. n), seed 0) for a whole frame of a large entry: mz_zs_xxh64 with sixteen stripes' loads
 * issued before their rounds.  The four accumulators are serial chains, but the loads do not depend on them: one load per
 * round leaves a lane waiting for memory at every stripe (64 MiB: 280 ms, 89 % of the call). */
MZ_DEV uint32_t mz_zsp_xxh64(const uint8_t *d, uint32_t n) {
    MZ_LANE_DECL
    uint64_t h;
    uint32_t i;
    if (n < 512u) return mz_zs_xxh64(d, n);
    {
        const uint32_t stripes = n >> 5;
        PV(uint32_t, lo);
        PV(uint32_t, hi);
        MZ_LANES {
            const uint32_t k = (uint32_t)lane & 3u;
            uint64_t v = k == 0 ? MZ_XXH_P1 + MZ_XXH_P2 : k == 1u ? MZ_XXH_P2 : k == 2u ? 0ull : 0ull - MZ_XXH_P1;
            if ((uint32_t)lane < 4u) {
                const uint8_t *q = d + 8u * k;
                uint32_t s = 0;
                for (; s + 16u <= stripes; s += 16u) {
                    uint64_t w[16];
                    MZ_ZSP_UNROLL
                    for (uint32_t j = 0; j < 16u; j++) w[j] = mz_ld8(q + 32u * (size_t)(s + j));
                    MZ_ZSP_UNROLL
                    for (uint32_t j = 0; j < 16u; j++) v = mz_xxh_round(v, w[j]);
                }
                for (; s < stripes; s++) v = mz_xxh_round(v, mz_ld8(q + 32u * (size_t)s));
            }
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

/* table `which` of a block from the definer the host named: the descriptions in front of it are read over, not built */
MZ_DEV uint32_t mz_zsp_table_from(mz_zs_ctx *C, mz_zs_lds *S, uint32_t which, uint32_t p, uint32_t modes, uint32_t end, uint32_t *al) {
    for (uint32_t w = 0; w < which; w++) {
        const uint32_t mode = (modes >> (6u - 2u * w)) & 3u;
        if (mode == 1u) {
            p += 1u;
        } else if (mode == 2u) {
            uint32_t a = 0, nsym = 0;
            const uint32_t used = mz_zs_fse_read(C, S, p, end, w == 1u ? 8u : 9u, w == 0 ? 35u : w == 1u ? 31u : 52u, &a, &nsym);
            if (used == MZ_ZS_ERR) return MZ_ZS_ERR;
            p += used;
        }
        if (p > end) return MZ_ZS_ERR;
    }
    {
        const uint32_t mode = (modes >> (6u - 2u * which)) & 3u;
        if (mode == 3u) return MZ_ZS_ERR; /* (a definer defines) */
        return mz_zs_seq_table(C, S, which, mode, p, end, al);
    }
}

/* one block: mode 1 counts (Compressed blocks only), mode 2 emits.  ptr is biased: ptr[i] belongs to out[i]. */
MZ_DEV void mz_zsp_block(const uint8_t *in, uint32_t in_len, const uint32_t *job, uint32_t mode, uint8_t *out, uint32_t *ptr, mz_zs_lds *S,
                         uint8_t *scratch, uint32_t *res) {
    MZ_LANE_DECL
    mz_zs_ctx ctx;
    mz_zs_ctx *const C = &ctx;
    const uint32_t off = MZ_UNIFORM(job[MZ_ZSP_J_OFF]), bs = MZ_UNIFORM(job[MZ_ZSP_J_SIZE]), type = MZ_UNIFORM(job[MZ_ZSP_J_TYPE]) & 3u;
    const uint32_t pos = MZ_UNIFORM(job[MZ_ZSP_J_POS]), oend = MZ_UNIFORM(job[MZ_ZSP_J_END]), fo = MZ_UNIFORM(job[MZ_ZSP_J_FO]);
    uint32_t bad = 1, o = pos, lit_n = 0, lp = 0, total = 0;
    uint32_t s0 = 0, s1 = 1, s2 = 2, v0 = 0, v1 = 0, v2 = 0; /* the repeat offsets as (source, value) */
    C->in = in;
    C->in_len = in_len;
    C->base = 0u - MZ_ZS_INBUF;
    C->out = out;
    C->out_cap = oend;
    C->lit = scratch;
    C->o = pos;
    C->fo = fo;
    C->blk_max = MZ_UNIFORM(job[MZ_ZSP_J_BLKMAX]);
    C->rep0 = C->rep1 = C->rep2 = 0;
    C->have_huf = C->huf_log = 0;
    C->have_seq = 1;
    C->al_ll = C->al_of = C->al_ml = 0;
    MZ_ZSPROF_INIT(C);
    if (mode == 2u) {
        s0 = s1 = s2 = 3u;
        v0 = MZ_UNIFORM(job[MZ_ZSP_J_REP0]);
        v1 = MZ_UNIFORM(job[MZ_ZSP_J_REP0 + 1]);
        v2 = MZ_UNIFORM(job[MZ_ZSP_J_REP0 + 2]);
    }
    if (off > in_len || 3u > in_len - off) goto done;
    if (type < 2u) { /* Raw, RLE: emit only */
        const uint32_t p = off + 3u;
        if (mode != 2u || bs != oend - pos || oend < pos) goto done;
        if (type == 0) {
            if (bs > in_len - p) goto done;
            MZ_LANES {
                for (uint32_t k = (uint32_t)lane; k < bs; k += 64u) {
                    out[pos + k] = in[p + k];
                    ptr[pos + k] = pos + k;
                }
            }
        } else {
            if (p >= in_len) goto done;
            const uint32_t v = mz_zs_byte(C, S, p);
            MZ_LANES {
                for (uint32_t k = (uint32_t)lane; k < bs; k += 64u) {
                    out[pos + k] = (uint8_t)v;
                    ptr[pos + k] = pos + k;
                }
            }
        }
        total = bs;
        bad = 0;
        goto done;
    }
    {
        const uint32_t end = off + 3u + bs;
        uint32_t p = off + 3u, used, b0, nseq;
        if (type != 2u || bs > in_len - p || bs < 3u) goto done;
        if (mode == 2u) {
            if (oend < pos) goto done;
            if ((mz_zs_byte(C, S, p) & 3u) == 3u) { /* treeless: the tree of the definer first */
                const uint32_t t0 = MZ_UNIFORM(job[MZ_ZSP_J_TREE]), t1 = MZ_UNIFORM(job[MZ_ZSP_J_TREE_END]);
                if (t1 > in_len || t0 >= t1) goto done;
                if (mz_zs_huf_read(C, S, t0, t1) == MZ_ZS_ERR) goto done;
            }
            used = mz_zs_literals(C, S, p, end, &lit_n);
            if (used == MZ_ZS_ERR || p + used != MZ_UNIFORM(job[MZ_ZSP_J_SEQ])) goto done;
            MZ_CHASE_FENCE(); /* literals are stored through some lanes' addresses and read through others' */
            MZ_WAVE_SYNC();
        } else {
            lit_n = MZ_UNIFORM(job[MZ_ZSP_J_REGEN]);
        }
        p = MZ_UNIFORM(job[MZ_ZSP_J_SEQ]);
        if (p >= end || p < off + 3u) goto done;
        b0 = mz_zs_byte(C, S, p);
        if (b0 < 128u) {
            nseq = b0;
            p += 1u;
        } else if (b0 < 255u) {
            if (end - p < 2u) goto done;
            nseq = ((b0 - 128u) << 8) + mz_zs_byte(C, S, p + 1u);
            p += 2u;
        } else {
            if (end - p < 3u) goto done;
            nseq = mz_zs_le(C, S, p + 1u, 2) + 0x7F00u;
            p += 3u;
        }
        if (nseq == 0) {
            if (p != end) goto done;
        } else {
            uint32_t modes, sll, sof, sml;
            mz_zs_bits B;
            if (p >= end) goto done;
            modes = mz_zs_byte(C, S, p);
            p += 1u;
            if (modes & 3u) goto done;
            for (uint32_t w = 0; w < 3u; w++) {
                const uint32_t m = (modes >> (6u - 2u * w)) & 3u;
                uint32_t *const al = w == 0 ? &C->al_ll : w == 1u ? &C->al_of : &C->al_ml;
                if (m == 3u) {
                    const uint32_t dp = MZ_UNIFORM(job[MZ_ZSP_J_DEF + 3u * w]), dm = MZ_UNIFORM(job[MZ_ZSP_J_DEF + 3u * w + 1u]);
                    const uint32_t de = MZ_UNIFORM(job[MZ_ZSP_J_DEF + 3u * w + 2u]);
                    if (de > in_len || dp > de || de == 0) goto done;
                    if (mz_zsp_table_from(C, S, w, dp, dm, de, al) == MZ_ZS_ERR) goto done;
                } else {
                    used = mz_zs_seq_table(C, S, w, m, p, end, al);
                    if (used == MZ_ZS_ERR) goto done;
                    p += used;
                }
            }
            if (!mz_zs_bits_open(C, S, &B, p, end - p)) goto done;
            sll = mz_zs_bits_read(C, S, &B, C->al_ll);
            sof = mz_zs_bits_read(C, S, &B, C->al_of);
            sml = mz_zs_bits_read(C, S, &B, C->al_ml);
            if (B.bits < 0) goto done;
            for (uint32_t i = 0; i < nseq; i++) {
                const uint32_t ell = MZ_UNIFORM(S->ll[sll]), eof = MZ_UNIFORM(S->of[sof]), eml = MZ_UNIFORM(S->ml[sml]);
                const uint32_t ofc = eof & 255u;
                uint32_t nb_ll, nb_ml, ll, ml, ofv;
                ofv = (1u << ofc) + mz_zs_bits_read(C, S, &B, ofc);
                ml = mz_zs_ml_base(eml & 255u, &nb_ml);
                ml += mz_zs_bits_read(C, S, &B, nb_ml);
                ll = mz_zs_ll_base(ell & 255u, &nb_ll);
                ll += mz_zs_bits_read(C, S, &B, nb_ll);
                if (i + 1u < nseq) {
                    sll = (ell >> 16) + mz_zs_bits_read(C, S, &B, (ell >> 8) & 255u);
                    sml = (eml >> 16) + mz_zs_bits_read(C, S, &B, (eml >> 8) & 255u);
                    sof = (eof >> 16) + mz_zs_bits_read(C, S, &B, (eof >> 8) & 255u);
                }
                if (B.bits < 0) goto done;
                /* ---- repeat offsets, concrete (emit) or as a function of the incoming ones (count) */
                if (ofv > 3u) {
                    s2 = s1;
                    v2 = v1;
                    s1 = s0;
                    v1 = v0;
                    s0 = 3u;
                    v0 = ofv - 3u;
                } else {
                    const uint32_t idx = ofv - 1u + (ll == 0u);
                    if (idx != 0) {
                        uint32_t ns, nv;
                        if (idx == 1u) {
                            ns = s1;
                            nv = v1;
                        } else if (idx == 2u) {
                            ns = s2;
                            nv = v2;
                        } else {
                            ns = s0;
                            nv = s0 == 3u ? v0 - 1u : v0 + 1u; /* rep0 - 1: k grows where the slot is still symbolic */
                        }
                        if (ns == 3u && nv == 0) goto done;
                        if (idx != 1u) {
                            s2 = s1;
                            v2 = v1;
                        }
                        s1 = s0;
                        v1 = v0;
                        s0 = ns;
                        v0 = nv;
                    }
                }
                if (ll > lit_n - lp) goto done;
                if (ll + ml > C->blk_max - (o - pos)) goto done; /* (o - pos <= blk_max: checked for every sequence before) */
                if (mode == 2u) {
                    const uint32_t m0 = o + ll, dist = v0;
                    if (ll + ml > oend - o) goto done;
                    if (dist == 0 || dist > m0 - fo) goto done;
                    {
                        const uint8_t *lit = C->lit + lp;
                        MZ_LANES {
                            for (uint32_t k = (uint32_t)lane; k < ll; k += 64u) {
                                out[o + k] = lit[k];
                                ptr[o + k] = o + k;
                            }
                            for (uint32_t k = (uint32_t)lane; k < ml; k += 64u) ptr[m0 + k] = m0 - dist + (dist < ml ? k % dist : k);
                        }
                    }
                }
                lp += ll;
                o += ll + ml;
            }
            if (B.bits != 0) goto done;
        }
        /* ---- the literals behind the last sequence */
        {
            const uint32_t n = lit_n - lp;
            if (n > C->blk_max - (o - pos)) goto done;
            if (mode == 2u) {
                const uint8_t *lit = C->lit + lp;
                if (n != oend - o) goto done; /* the block ends where the count pass said */
                MZ_LANES {
                    for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
                        out[o + k] = lit[k];
                        ptr[o + k] = o + k;
                    }
                }
            }
            o += n;
        }
        total = o - pos;
        bad = 0;
    }
done:
    res[MZ_ZSP_O_STATUS] = bad;
    res[MZ_ZSP_O_BYTES] = total;
    res[MZ_ZSP_O_REP + 0] = s0;
    res[MZ_ZSP_O_REP + 1] = v0;
    res[MZ_ZSP_O_REP + 2] = s1;
    res[MZ_ZSP_O_REP + 3] = v1;
    res[MZ_ZSP_O_REP + 4] = s2;
    res[MZ_ZSP_O_REP + 5] = v2;
}

#endif
