/* inflate_emit.inc -- the second half of K1's chase window (inflate_chase.inc): the records of the chain become bytes.
 *   emit     the records are taken MZ_EMIT_GROUP at a time by 64 lanes in stream order (a lane finds its group by a binary
 *            search in the prefix sums of the lanes' group counts, tables in LDS), counted, prefix-summed, cut where the
 *            pool is full and written as staging bytes / back-reference pieces of <= 32 bytes, each piece classed by where its
 *            source lies and entered in the far list, the near list, or (split) both;
 *   commit   inflate_commit.inc: far copies (sources older than the chunk, from the output buffer), near copies (sources
 *            inside the chunk, in dependency order), the store, the CRC-32 fold.
 * A function of its own, not inlined (see inflate_walk.inc): what it keeps alive is the round's records and counters, not
 * the entry's cursor, block and resume state.  Replaces, per window, the copy loops of zlib's inflate_fast() and the
 * mz_crypt_crc32_update behind mz_zip_entry_read (mz_zip.c:2049). */
/* the lane's group of the round that starts at group G0_ of the chain: P(w)[] = its records (mz_chase_step), 0 where a slot is not the chain's; P(kq)[] = their bits | bytes the
 * token produces << 8, 0 = no record.  Expects tab_n / tab_e / tab_m / tab_g (LDS), Rp / Cp / Lp / Lc, NG.
 * (The fetch half for the next round asked for as soon as this round's cut is known: 13 registers held across the commit, 40 -> 112 / 128
 * bytes of scratch for 0.6 % with overlapping ranges: profiles/r7, DESIGN.md section 3 K1) */
#define MZ_EMIT_LOAD_GROUP(G0_) \
        { \
            PV2(uint32_t, fw_, MZ_EMIT_GROUP); \
            PV(uint32_t, fk0_); \
            PV(uint32_t, fk1_); \
            PV(uint32_t, flo_); \
            PV(uint32_t, fhi_); \
            PV(uint32_t, fst_); \
            /* the search for the lane's group and the loads of its raw records (fw_), step bytes (fk0_, fk1_) and slot range (flo_, fhi_, fst_) */ \
            MZ_LANES { \
                const uint32_t G = (G0_) + (uint32_t)lane; \
                uint32_t lo = 0, hi_ = 0, st0 = 0; \
                uint32_t kw0 = 0, kw1 = 0; \
_Pragma("unroll") \
                for (uint32_t k = 0; k < MZ_EMIT_GROUP; k++) P(fw_)[k] = 0u; \
                if (G < NG) { \
                    uint32_t j = 0; /* the first lane whose inclusive sum exceeds G */ \
_Pragma("unroll") \
                    for (uint32_t sp = 32u; sp; sp >>= 1) \
                        if (tab_g[j + sp - 1u] <= G) j += sp; \
                    const uint32_t k = G - (j ? tab_g[j - 1u] : 0u); \
                    const uint32_t n = tab_n[j], e = tab_e[j], m = tab_m[j]; \
                    const uint32_t ts = e & 0x7FFFu; \
                    const uint32_t cr = (n > ts) ? ((n + MZ_EMIT_GROUP - 1u) / MZ_EMIT_GROUP) - ts / MZ_EMIT_GROUP : 0u; \
                    const uint8_t *base, *kbase; \
                    if (k < cr) { /* (a lane is always met at the START of one of its steps: no half records) */ \
                        st0 = (ts / MZ_EMIT_GROUP + k) * MZ_EMIT_GROUP; \
                        lo = (ts > st0) ? ts : st0; \
                        hi_ = (n < st0 + MZ_EMIT_GROUP) ? n : st0 + MZ_EMIT_GROUP; \
                        base = Rp; \
                        kbase = Lp + j * MZ_REC_CAP1; \
                    } else { \
                        st0 = (k - cr) * MZ_EMIT_GROUP; \
                        lo = st0; \
                        hi_ = (m < st0 + MZ_EMIT_GROUP) ? m : st0 + MZ_EMIT_GROUP; \
                        base = Cp; \
                        kbase = Lc + j * MZ_REC_CAP2; \
                    } \
_Pragma("unroll") \
                    for (uint32_t pp = 0; pp < MZ_EMIT_GROUP / 4u; pp++) { \
                        mz_dw4 v; \
                        __builtin_memcpy(&v, base + MZ_REC_ADDR(st0 / 4u + pp, j), 16); \
                        P(fw_)[4u * pp] = v.v[0]; \
                        P(fw_)[4u * pp + 1u] = v.v[1]; \
                        P(fw_)[4u * pp + 2u] = v.v[2]; \
                        P(fw_)[4u * pp + 3u] = v.v[3]; \
                    } \
                    { \
                        const uint64_t kk = mz_ld8(kbase + st0); \
                        kw0 = (uint32_t)kk; \
                        kw1 = (uint32_t)(kk >> 32); \
                    } \
                } \
                P(fk0_) = kw0; \
                P(fk1_) = kw1; \
                P(flo_) = lo; \
                P(fhi_) = hi_; \
                P(fst_) = st0; \
            } \
            /* P(w)[], P(kq)[] from them */ \
            MZ_LANES { \
                /* slots that are not the chain's hold nothing from here on */ \
_Pragma("unroll") \
                for (uint32_t r = 0; r < MZ_EMIT_GROUP; r++) { \
                    const uint32_t st = P(fst_) + r; \
                    const uint32_t kb = mz_bfe((r & 4u) ? P(fk1_) : P(fk0_), 8u * (r & 3u), 8); \
                    const uint32_t in = (st >= P(flo_) && st < P(fhi_) && kb != 0u) ? 1u : 0u; \
                    const uint32_t ln = (kb < MZ_K_LIT) ? mz_bfe(P(fw_)[r], 8, 8) + 3u : (kb < MZ_K_EOB) ? 1u : 0u; \
                    P(w)[r] = in ? P(fw_)[r] : 0u; \
                    P(kq)[r] = in ? ((kb & 63u) | (ln << 8)) : 0u; \
                } \
            } \
        }

typedef struct mz_emit_result {
    uint32_t out_pos, crc_done;
    uint32_t cbits; /* bits of the records that were committed */
    uint32_t fail;  /* a round could not be committed here (capacity, a distance in front of the entry): the step loop has the verdict */
    uint32_t all;   /* every group of the chain was taken */
    PV(uint32_t, crc_acc);
} mz_emit_result;
MZ_DEV_NOINLINE mz_emit_result mz_chase_emit(mz_lds_handle L_, uint32_t sub_used_, mz_glb_handle rec_, mz_glb_handle out_, uint32_t out_pos_,
                                             uint32_t out_cap_, uint32_t NG_, uint32_t crc_base_, uint32_t crc_done_, PVIN(uint32_t, crc_acc_in),
                                             mz_lds_handle crc_tab_, mz_glb_handle tabs_ MZ_PROF_PARAMS) {
    MZ_LANE_DECL
    /* wave-uniform arguments, back in scalar registers (wave.h, MZ_UNIFORM64) */
    const uint32_t sub_used = MZ_UNIFORM(sub_used_), out_cap = MZ_UNIFORM(out_cap_), NG = MZ_UNIFORM(NG_), crc_base = MZ_UNIFORM(crc_base_);
    uint32_t out_pos = MZ_UNIFORM(out_pos_), crc_done = MZ_UNIFORM(crc_done_);
    mz_inflate_lds *const L = MZ_LDS_FROM(mz_inflate_lds, L_);
    uint8_t *const rec = MZ_GLB_FROM(uint8_t, rec_);
    uint8_t *const out = MZ_GLB_FROM(uint8_t, out_);
    const uint32_t *const crc_tab = MZ_LDS_FROM(const uint32_t, crc_tab_);
    const mzhip_crc_tables *const tabs = MZ_GLB_FROM(const mzhip_crc_tables, tabs_);
    PV(uint32_t, crc_acc);
    MZ_LANES { P(crc_acc) = P(crc_acc_in); }
    uint32_t *const pool0 = L->lit_sub + ((sub_used + 3u) & ~3u);
    uint8_t *const stg = (uint8_t *)pool0;
    uint32_t *const ring = MZ_L_WIN(L);
    uint32_t *const tab_n = ring + 64u * MZ_CRING_RS - 256u, *const tab_e = tab_n + 64, *const tab_m = tab_n + 128, *const tab_g = tab_n + 192;
    uint32_t *const lst = tab_n; /* entry j: lst[-(j + 1)], see inflate_commit.inc */
    const uint32_t pool_bytes = (uint32_t)((uint8_t *)lst - stg);
    uint8_t *const Rp = rec;
    uint8_t *const Cp = rec + MZ_REC_AREA(MZ_REC_CAP1);
    uint8_t *const Lp = Cp + MZ_REC_AREA(MZ_REC_CAP2);
    uint8_t *const Lc = Lp + 64u * MZ_REC_CAP1;
    uint32_t G0 = 0; /* the next group of the chain */
    uint32_t cbits = 0;         /* bits of the records committed so far */
    uint32_t fail = 0;
    PV(uint32_t, bad);
    while (G0 < NG) {
        MZ_STAT(9, 1);
        const uint32_t sb = (uint32_t)((uintptr_t)(out + out_pos) & 15u);
        PV2(uint32_t, w, MZ_EMIT_GROUP);  /* the lane's records (mz_chase_step), 0 where the slot is not the chain's */
        PV2(uint32_t, kq, MZ_EMIT_GROUP); /* ... their bits | bytes the token produces << 8; 0 = no record */
        MZ_EMIT_LOAD_GROUP(G0)
        /* what the lane's records produce: bytes, pieces, bits */
#define MZ_CHASE_REC(r_, in_, rc_, ln_)                                                      \
        const uint32_t rc_ = P(w)[(r_)];                                                     \
        const uint32_t in_ = P(kq)[(r_)] ? 1u : 0u;                                          \
        const uint32_t ln_ = P(kq)[(r_)] >> 8;
        PV(uint32_t, lby);
        PV(uint32_t, lbt);
        MZ_LANES {
            uint32_t by = 0, bt = 0;
#pragma unroll
            for (uint32_t r = 0; r < MZ_EMIT_GROUP; r++) {
                MZ_CHASE_REC(r, in, rc, ln)
                (void)in;
                by += ln + (rc >> 31);
                bt += P(kq)[r] & 63u;
            }
            P(lby) = by;
            P(lbt) = bt;
        }
        PV(uint32_t, sib);
        MZ_INCL_SCAN(sib, lby);
        /* Every piece of <= 32 bytes is classed by where its source lies, now that the byte scan has placed it: dw = its
         * offset in the chunk (staging index - sb), nfar = min(max(dist - dw, 0), len) of its bytes are older than the chunk.
         *   far only    nfar == len   one far entry;
         *   near only   nfar == 0     one near entry;
         *   split       otherwise     a far entry for the first nfar bytes and a near entry for the rest, at staging index
         *                             + nfar with the same distance.
         * A match of L bytes (pieces at 32 k, all with the match's distance) has nfar = min(max(dist - dw, 0), L) far bytes in
         * front: (nfar + 31) / 32 of its pieces have a far part, and, when nfar < L, all but its first nfar / 32 a near one.
         * The two counts of a lane are summed together, far | near << 16 (a round holds at most 64 x 8 x 10 entries). */
#define MZ_CHASE_NFAR(dist_, dw_, ln_) (((dist_) > (dw_)) ? (((dist_) - (dw_) < (ln_)) ? (dist_) - (dw_) : (ln_)) : 0u)
        PV(uint32_t, lfn);
        MZ_LANES {
            uint32_t dw = P(sib) - P(lby), fn = 0;
#pragma unroll
            for (uint32_t r = 0; r < MZ_EMIT_GROUP; r++) {
                MZ_CHASE_REC(r, in, rc, ln)
                (void)in;
                dw += rc >> 31;
                if (ln > 1u) {
                    const uint32_t dist = mz_bfe(rc, 16, 15) + 1u;
                    const uint32_t nfar = MZ_CHASE_NFAR(dist, dw, ln);
                    fn += ((nfar + 31u) >> 5) + ((nfar < ln) ? (((ln + 31u) >> 5) - (nfar >> 5)) << 16 : 0u);
                }
                dw += ln;
            }
            P(lfn) = fn;
        }
        PV(uint32_t, sfn);
        MZ_INCL_SCAN(sfn, lfn);
        /* what fits the pool: staging bytes from the front, 4 bytes per list entry (far and near) from the back, 12 bits of
         * staging index.  The need is exact: split pieces are counted twice.  Both sums are monotone, so the lanes that fit
         * entirely are a run from lane 0, and a round with many split pieces only takes fewer lanes. */
#define MZ_CHASE_FITS(B_, M_) ((B_) <= 4096u && (B_) + 4u * (M_) + 48u <= pool_bytes)
        uint64_t nofit;
        MZ_BALLOT(nofit, !MZ_CHASE_FITS(sb + P(sib), (P(sfn) & 0xFFFFu) + (P(sfn) >> 16)));
        /* the round takes whole lanes: lanes 0 .. cut - 1 (lane 0's eight records always fit an empty pool, with every piece
         * that can be split split: 15 + 8 x 259 bytes and 8 x (9 + 1) entries -- the pieces of one match share its distance,
         * so at most one of them is split -- are 2 087 + 320 + 48 = 2 455 bytes of the >= 5 104 a pool has).  Round 4 let the
         * cut lane take a prefix of its records, counted once more record by record in every lane on every round: ~100
         * instructions a round to fill the pool's last 26 bytes */
        const uint32_t cut = nofit ? mz_ctz64(nofit) : 64u;
        PV(uint32_t, acc); /* record slots of this lane that are taken */
        uint32_t Tb, Tfar, Tnear, Tbits;
        MZ_LANES {
            P(acc) = ((uint32_t)lane < cut) ? MZ_EMIT_GROUP : 0u;
            if ((uint32_t)lane >= cut) P(lbt) = 0u;
        }
        Tb = MZ_READLANE(sib, (cut ? cut : 1u) - 1u);
        {
            const uint32_t t = MZ_READLANE(sfn, (cut ? cut : 1u) - 1u);
            Tfar = t & 0xFFFFu;
            Tnear = t >> 16;
        }
#undef MZ_CHASE_FITS
        MZ_WAVE_SUM(Tbits, lbt);
        if (cut == 0u || Tbits == 0u || Tb > out_cap - out_pos) {
            /* (a lane's records always fit an empty pool, so no bits = a bug;) output beyond the entry's capacity: the step loop decides the verdict */
            fail = 1;
            break;
        }
        /* write the round: literals to their staging byte, back-references as pieces of <= 32 bytes */
        /* Near entries at lst[-(j + 1)], j < Tnear, in stream order (the lane's first index is its exclusive sum: the rank
         * searches of the near stage rely on sorted starts and ends); far entries behind them at lst[-(Tnear + f + 1)],
         * f < Tfar, in whatever order the same sums give.  A piece of p_ bytes at staging index i_, its first f_ bytes far: */
#define MZ_CHASE_PIECE(i_, p_, f_)                                                                          \
        {                                                                                                   \
            const uint32_t pf_ = ((f_) < (p_)) ? (f_) : (p_);                                               \
            MZ_STAT(21, (pf_ != 0u && pf_ < (p_)) ? 1u : 0u); /* a piece split between far and near (counted where it is  \
                                                                 classed: also in a round that P(bad) then refuses) */      \
            if (pf_ != 0u) lst[-(int32_t)(++fi)] = (i_) | ((pf_ - 1u) << 12) | dd;                          \
            if (pf_ < (p_)) lst[-(int32_t)(++ni)] = ((i_) + pf_) | (((p_) - pf_ - 1u) << 12) | dd;          \
        }
        MZ_LANES {
            uint32_t bd = 0;
            uint32_t pos = sb + P(sib) - P(lby);
            uint32_t fi = Tnear + ((P(sfn) - P(lfn)) & 0xFFFFu), ni = (P(sfn) - P(lfn)) >> 16; /* entries in front of the lane's */
#pragma unroll
            for (uint32_t r = 0; r < MZ_EMIT_GROUP; r++) {
                MZ_CHASE_REC(r, in, rc, ln)
                if (in && r < P(acc)) {
                    if (rc >> 31) stg[pos++] = (uint8_t)rc;
                    if (ln == 1u) {
                        stg[pos] = (uint8_t)(rc >> 8);
                    } else if (ln > 1u) {
                        const uint32_t dist = mz_bfe(rc, 16, 15) + 1u, dd = (dist - 1u) << 17;
                        const uint32_t dw = pos - sb;
                        const uint32_t nfar = MZ_CHASE_NFAR(dist, dw, ln);
                        bd |= (dist > out_pos + dw) ? 1u : 0u; /* invalid distance too far back */
                        MZ_CHASE_PIECE(pos, (ln < 32u) ? ln : 32u, nfar)
                        /* the other pieces of a match of more than 32 bytes, same distance, in a branch of those lanes alone: 3.4 %
                         * of the bench corpus's matches at level 6 are that long, and 94 % of its chunks hold one */
                        if (ln > 32u) {
                            MZ_NOUNROLL
                            for (uint32_t o = 32u; o < ln; o += 32u) MZ_CHASE_PIECE(pos + o, (ln - o < 32u) ? ln - o : 32u, (nfar > o) ? nfar - o : 0u)
                        }
                    }
                    pos += ln;
                }
            }
            P(bad) = bd;
        }
#undef MZ_CHASE_PIECE
#undef MZ_CHASE_NFAR
#undef MZ_CHASE_REC
        MZ_PROF_MARK(13); /* emit */
#include "inflate_commit.inc"
        if (fail) break;
        cbits += Tbits;
        G0 += cut;
    }
    mz_emit_result er;
    er.out_pos = out_pos;
    er.crc_done = crc_done;
    er.cbits = cbits;
    er.fail = fail;
    er.all = (G0 >= NG) ? 1u : 0u;
    MZ_LANES { P(er.crc_acc) = P(crc_acc); }
    return er;
}

/* ---- the records of a window WITHOUT stream order (one large entry decoded by many waves, mzhip_inflate_parallel_host) ----
 * When every DEFLATE block of a window of a large entry is parsed by a wave of its own, a block's back-references cannot be
 * copied yet: the bytes they point at belong to blocks other waves are still working on.  So the records are not turned
 * into bytes here but into a SOURCE MAP: a literal goes to out[] and points at itself, byte k of a match points at the byte
 * `distance` in front of it.  k_ptr_jump then halves every chain of pointers per round (ptr[i] = ptr[ptr[i]]) until all
 * point at literals -- or at the history in front of the window, which is final --, and k_ptr_gather fetches the bytes.
 * mode 1 only counts what the window produces (the blocks' output positions are a prefix sum over those counts), mode 2
 * writes.  `pos0` = index in out[] / ptr[] of the window's first byte (history included).  Returns the bytes produced;
 * bad: a distance that reaches in front of out[0]. */
typedef struct mz_ptr_result {
    uint32_t bytes, bad;
} mz_ptr_result;
MZ_DEV_NOINLINE mz_ptr_result mz_chase_emit_ptr(mz_lds_handle L_, mz_glb_handle rec_, uint32_t NG_, uint32_t mode_, mz_glb_handle out_,
                                                mz_glb_handle ptr_, uint32_t pos0_) {
    MZ_LANE_DECL
    const uint32_t NG = MZ_UNIFORM(NG_), mode = MZ_UNIFORM(mode_), pos0 = MZ_UNIFORM(pos0_);
    mz_inflate_lds *const L = MZ_LDS_FROM(mz_inflate_lds, L_);
    uint8_t *const rec = MZ_GLB_FROM(uint8_t, rec_);
    uint8_t *const out = MZ_GLB_FROM(uint8_t, out_);
    uint32_t *const ptr = MZ_GLB_FROM(uint32_t, ptr_);
    uint32_t *const ring = MZ_L_WIN(L);
    uint32_t *const tab_n = ring + 64u * MZ_CRING_RS - 256u, *const tab_e = tab_n + 64, *const tab_m = tab_n + 128, *const tab_g = tab_n + 192;
    uint8_t *const Rp = rec;
    uint8_t *const Cp = rec + MZ_REC_AREA(MZ_REC_CAP1);
    uint8_t *const Lp = Cp + MZ_REC_AREA(MZ_REC_CAP2);
    uint8_t *const Lc = Lp + 64u * MZ_REC_CAP1;
    uint32_t total = 0, badany = 0;
    for (uint32_t G0 = 0; G0 < NG; G0 += 64u) {
        PV2(uint32_t, w, MZ_EMIT_GROUP);
        PV2(uint32_t, kq, MZ_EMIT_GROUP);
        MZ_EMIT_LOAD_GROUP(G0)
        PV(uint32_t, lby);
        PV(uint32_t, sib);
        MZ_LANES {
            uint32_t by = 0;
#pragma unroll
            for (uint32_t r = 0; r < MZ_EMIT_GROUP; r++) by += (P(kq)[r] >> 8) + (P(w)[r] >> 31);
            P(lby) = by;
        }
        MZ_INCL_SCAN(sib, lby);
        if (mode == 2u) {
            PV(uint32_t, bad);
            MZ_LANES {
                uint32_t pos = pos0 + total + P(sib) - P(lby), bd = 0;
                for (uint32_t r = 0; r < MZ_EMIT_GROUP; r++) {
                    const uint32_t rc = P(w)[r], ln = P(kq)[r] >> 8;
                    if (P(kq)[r]) {
                        if (rc >> 31) {
                            out[pos] = (uint8_t)rc;
                            ptr[pos] = pos;
                            pos++;
                        }
                        if (ln == 1u) {
                            out[pos] = (uint8_t)(rc >> 8);
                            ptr[pos] = pos;
                        } else if (ln > 1u) {
                            const uint32_t dist = mz_bfe(rc, 16, 15) + 1u;
                            if (dist > pos) {
                                bd = 1u;
                            } else {
                                MZ_NOUNROLL
                                for (uint32_t k = 0; k < ln; k++) ptr[pos + k] = pos + k - dist;
                            }
                        }
                        pos += ln;
                    }
                }
                P(bad) = bd;
            }
            uint64_t bm;
            MZ_BALLOT(bm, P(bad) != 0u);
            if (bm) badany = 1u;
        }
        total += MZ_READLANE(sib, 63);
    }
    MZ_WAVE_SYNC();
    mz_ptr_result r;
    r.bytes = total;
    r.bad = badany;
    return r;
}
