/* inflate_commit.inc -- one chunk of K1's span path leaves LDS: far copies, near copies, store, CRC.
 * Textually included by inflate_emit.inc (mz_chase_emit) after the emit wrote the chunk into the pool:
 *   literals      at their staging byte (stg[sb + r] <-> out[out_pos + r], sb = the 16-byte misalignment of out + out_pos),
 *   back-refs     as list entries of two lists, staging index (12 bits) | (length - 1) << 12 (5 bits, pieces of at most 32
 *                 bytes) | (distance - 1) << 17: the near list lst[-(j + 1)], j < Tnear, in stream order (sources inside
 *                 the chunk), and behind it the far list lst[-(Tnear + f + 1)], f < Tfar, in no order (sources older than
 *                 the chunk).  A piece that is part far, part near is an entry of each.
 * Expects (wave-uniform) sb, Tb = bytes of the chunk, Tfar / Tnear = list entries, stg, lst, pool0, P(bad) (a lane saw a
 * distance reaching in front of the entry) and `fail`; on success the bytes are in out[], out_pos has moved and the CRC is
 * folded that far; with fail set nothing has left LDS.
 *   far       the entries of the far list are fetched from the output buffer, 64 at a time, each lane its own, with up
 *             to four 8-byte loads in flight;
 *   near      64 entries of the near list at a time; a piece is copied (8 bytes per step, LDS to LDS) as soon as
 *             no piece that writes a byte of its source is unfinished -- the rounds follow the true dependency depth
 *             inside the batch (tests/study/flush_rounds.c);
 *   store     16 bytes per lane, head and tail bytes by single lanes.
 * (Measured and dropped: two far pieces per lane in flight, near copies with all loads first, two near pieces per lane: each
 * 3.6 - 4.4 % SLOWER in round 5, profiles/r5/call1_probe.log -- and again once the wave's control had become scalar: loads
 * first -5 %, two far batches in flight +0.9 % on 64 KiB entries and -1.8 % on 8 KiB, call15 / call16 -- more instructions
 * buy nothing here, the kernel is bound by issue slots) */
{
    MZ_WAVE_SYNC();
    uint8_t *const gdst = out + out_pos;
    MZ_STAT(10, Tb); MZ_STAT(12, Tfar + Tnear); MZ_STAT(15, 1);
    {
        uint64_t badm;
        MZ_BALLOT(badm, P(bad) != 0u);
        if (badm) fail = 1; /* nothing of the chunk has left LDS: the step loop meets the token and reports it in stream order */
    }
    /* far: the far list alone.  Its entries write staging bytes of their own and read only the output buffer, so one
     * MZ_WAVE_SYNC behind the whole stage is enough: it is for the near pieces, which read bytes that far pieces wrote.
     * (Every entry through a far batch that wrote its near rest back to the list, compacted: 435.3 - 442.8 against 444.7 - 452.0
     * GiB/s on config 2, profiles/r12; fe43378 is the last commit that builds it) */
    const uint32_t nnear = Tnear;
    for (uint32_t b = 0; b < Tfar && !fail; b += 64u) {
        MZ_STAT(26, 1); /* far batches */
#if !(MZ_ABLATE & 3)
        MZ_LANES {
            const uint32_t j = b + (uint32_t)lane;
            if (j < Tfar) {
                mz_piece32 pc;
                const uint32_t en = lst[-(int32_t)(Tnear + j + 1u)];
                const uint32_t si = en & 0xFFFu, nf = mz_bfe(en, 12, 5) + 1u, dist = (en >> 17) + 1u;
                mz_copy32_load(&pc, gdst - (dist - (si - sb)) /* >= out: checked in the emit; nf <= dist - (si - sb) */, nf);
                mz_copy32_store(&pc, stg + si, nf);
            }
        }
#endif
    }
    MZ_WAVE_SYNC();
    MZ_STAT(13, nnear);
    MZ_PROF_MARK(6); /* far */
    /* near: sources inside the chunk, in dependency order.  The pieces of a batch lie in stream order, so the ones whose
     * output a piece reads are a run of lanes [ca, cb): ca = pieces that end at or before its source, cb = pieces that
     * start before its source's end -- two rank queries in the sorted starts / ends, six cross-lane steps each.  A piece
     * is copied in the round in which none of that run is unfinished: the test is a mask against the ballot of the
     * unfinished, and finishing is the ballot's update (rounds 1 - 4 kept a bit per staged byte in LDS: two atomics per
     * piece to set, two reads per piece and round to test, two atomics to clear -- the same rounds, tests/emul counts them,
     * +0.7 % on the device: profiles/r5/call14_probe.log) */
#if !(MZ_ABLATE & 1)
    for (uint32_t b = 0; b < nnear && !fail; b += 64u) {
        MZ_STAT(25, 1); /* near batches */
        PV(uint32_t, d0);
        PV(uint32_t, rem);
        PV(uint32_t, dist);
        PV(uint32_t, kst); /* start of the piece's output, 0xFFFFFFFF in lanes without a piece */
        PV(uint32_t, ken); /* its end */
        PV(uint32_t, ca);
        PV(uint32_t, cb);
        PV(uint64_t, dep);
        MZ_LANES {
            const uint32_t j = b + (uint32_t)lane;
            uint32_t a = 0, rm = 0, ds = 0;
            if (j < nnear) {
                const uint32_t en = lst[-(int32_t)(j + 1u)];
                a = en & 0xFFFu;
                rm = mz_bfe(en, 12, 5) + 1u;
                ds = (en >> 17) + 1u;
            }
            P(d0) = a;
            P(rem) = rm;
            P(dist) = ds;
            P(kst) = rm ? a : 0xFFFFFFFFu;
            P(ken) = rm ? a + rm : 0xFFFFFFFFu;
            P(ca) = 0u;
            P(cb) = 0u;
        }
        /* The two searches keep ca and cb as BYTE offsets of the cross-lane gather (4 * rank: what ds_bpermute takes), so
         * a step is add, gather, compare, add per query and nothing is shifted or masked on the way; the first step asks
         * every lane for lane 31, which is a scalar read.  (One gather per step cannot serve both queries, packed keys or
         * not: after the first step ca and cb of a lane stand at different ranks, and a gather hands a lane the register
         * of ONE other lane.)
         * (Ranks as lane indices, shifted and masked for every gather, and the prologue below by a division: 0.35 % slower,
         * set-up loop 172 against 143 instructions: profiles/r10, DESIGN.md section 3 K1) */
        {
            PV(uint32_t, s0);
            PV(uint32_t, s1);
            const uint32_t ke31 = MZ_READLANE(ken, 31), ks31 = MZ_READLANE(kst, 31);
            MZ_LANES {
                /* the part of the source that is not this piece's own output */
                P(s0) = P(d0) - P(dist);
                P(s1) = P(s0) + ((P(rem) < P(dist)) ? P(rem) : P(dist));
                P(ca) = (ke31 <= P(s0)) ? 128u : 0u;
                P(cb) = (ks31 < P(s1)) ? 128u : 0u;
            }
#pragma unroll
            for (uint32_t step = 64u; step != 2u; step >>= 1) { /* 4 * (16, 8, 4, 2, 1) */
                PV(uint32_t, va);
                PV(uint32_t, vb);
                MZ_GATHER4(va, ken, P(ca) + (step - 4u));
                MZ_GATHER4(vb, kst, P(cb) + (step - 4u));
                MZ_LANES {
                    if (P(va) <= P(s0)) P(ca) += step;
                    if (P(vb) < P(s1)) P(cb) += step;
                }
            }
            MZ_LANES {
                P(ca) >>= 2;
                P(cb) >>= 2;
            }
        }
        MZ_LANES {
            /* (cb <= lane: a piece's source ends where its output starts at the latest) */
            P(dep) = (P(cb) > P(ca)) ? ((~0ull >> (64u - (P(cb) - P(ca)))) << P(ca)) : 0ull;
        }
        uint64_t U;
        MZ_BALLOT(U, P(rem) != 0u);
        MZ_STAT_ZERO(11); /* rounds of this batch; 24 = the most a batch took */
        while (U) {
            MZ_STAT(14, 1); MZ_STAT(11, 1); MZ_STAT_MAX(24, 11);
            uint64_t R;
            MZ_BALLOT(R, P(rem) != 0u && (P(dep) & U) == 0ull);
            if (!R) { /* cannot happen: the first unfinished piece of the chunk only reads finished bytes */
                MZ_STAT(22, 1);
                fail = 1;
                break;
            }
            MZ_LANES {
                if (P(rem) != 0u && (P(dep) & U) == 0ull) {
                    uint8_t *d = stg + P(d0);
                    uint32_t n = P(rem), D = P(dist);
                    if (D < 8u) {
                        /* short period: byte by byte until a multiple of the period reaches 8, then the
                         * same 8-byte steps at that distance (every byte equals the one D' behind it) */
                        /* D8 = D * ((7 + D) / D), the first multiple of D from 8 on: D8 - D for D = 1 .. 7 is 7, 6, 6, 4, 5, 6, 7
                         * (D8 = 8, 8, 9, 8, 10, 12, 14), a nibble each of one constant, where the quotient is a division by a
                         * variable (a reciprocal sequence on the device) */
                        const uint32_t D8 = D + ((0x76546670u >> (4u * D)) & 15u);
                        uint32_t pro = D8 - D;
                        if (pro > n) pro = n;
                        for (uint32_t k = 0; k < pro; k++) d[k] = d[(int32_t)k - (int32_t)D];
                        d += pro;
                        n -= pro;
                        D = D8;
                    }
                    mz_copy32_seq(d, d - D, n);
                    P(rem) = 0u;
                }
            }
            MZ_WAVE_SYNC();
            U &= ~R;
        }
    }
#endif
    MZ_PROF_MARK(7); /* near */
    if (!fail) {
        /* store: 16 bytes per lane, the ragged ends byte by byte */
#if !(MZ_ABLATE & 8)
        {
            const uint32_t e = sb + Tb;
            const uint32_t a0 = sb ? 16u : 0u, a1 = e & ~15u;
            uint8_t *const gal = gdst - sb; /* 16-byte aligned; gal[i] <-> stg[i] */
            const uint32_t hn = ((a0 < e) ? a0 : e) - sb;
            const uint32_t t0 = (a1 > a0) ? a1 : a0;
            const uint32_t tn = (e > t0) ? e - t0 : 0u;
            MZ_LANES {
                if ((uint32_t)lane < hn) gal[sb + (uint32_t)lane] = stg[sb + (uint32_t)lane];
                if ((uint32_t)lane < tn) gal[t0 + (uint32_t)lane] = stg[t0 + (uint32_t)lane];
                for (uint32_t c = a0 + 16u * (uint32_t)lane; c + 16u <= a1; c += 1024u) {
                    const uint64_t v0 = mz_ld8(stg + c), v1 = mz_ld8(stg + c + 8u);
                    mz_st8(gal + c, v0);
                    mz_st8(gal + c + 8u, v1);
                }
            }
        }
#endif
        MZ_WAVE_SYNC();
        out_pos += Tb;
        MZ_PROF_MARK(8); /* store */
#if !(MZ_ABLATE & 4)
        MZ_CRC_FOLD_SUPER_BT_GROUP(crc_acc, crc_done, out + crc_base, out_pos - crc_base, crc_tab, tabs->kx4);
#endif
        MZ_PROF_MARK(9); /* crc */
    }
}
