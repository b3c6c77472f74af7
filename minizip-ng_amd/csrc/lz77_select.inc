/* lz77_select.inc -- one step of 64 positions: select the tokens of the chain start, f(start), f(f(start)), ... by pointer
 * doubling, with no serial walk.  Textually included by deflate_select.inc (K4) and by mz_lz_tokenize() (K6,
 * lzma_enc_core.h) with P(pk) = every position's token ([8:0] match length or 0, the distance or the literal byte above),
 * P(g1) = its successor word (lz77_core.h mz_lz_succ), nv = valid positions, skip = positions of this step that the
 * previous step's last token covers.  Leaves ntok = tokens of the step and P(tpk) = those tokens, compacted into lanes
 * 0 .. ntok - 1, and skip moved on.  MZ_LZ_SELECT_MARK is the includer's: a statement that stands between the selection
 * and the gather of the tokens (K4's section mark; nothing in K6). */
            /* greedy selection: lane r <- r-th element of the chain start, f(start), f(f(start)), ... */
            PV(uint32_t, g2);
            PV(uint32_t, g4);
            PV(uint32_t, g8);
            PV(uint32_t, g16);
            PV(uint32_t, g32);
            PV(uint32_t, gt);
            PV(uint32_t, ct);
            PV(uint32_t, cpos);
            MZ_LANES { P(cpos) = (skip >= nv) ? (0x1000u | (4u * skip)) : (4u * skip); }
#define MZ_LZ_ROUND(gin, gout, bit)                                                          \
    MZ_GATHER4(gt, gin, P(gin));                                                             \
    MZ_GATHER4(ct, gin, P(cpos));                                                            \
    MZ_LANES {                                                                               \
        P(gout) = (P(gin) & 0x1000u) ? P(gin) : P(gt);                                       \
        P(cpos) = (((uint32_t)lane & (bit)) && !(P(cpos) & 0x1000u)) ? P(ct) : P(cpos);      \
    }
            MZ_LZ_ROUND(g1, g2, 1u)
            MZ_LZ_ROUND(g2, g4, 2u)
            MZ_LZ_ROUND(g4, g8, 4u)
            MZ_LZ_ROUND(g8, g16, 8u)
            MZ_LZ_ROUND(g16, g32, 16u)
            MZ_GATHER4(ct, g32, P(cpos));
            MZ_LANES { P(cpos) = (((uint32_t)lane & 32u) && !(P(cpos) & 0x1000u)) ? P(ct) : P(cpos); }
#undef MZ_LZ_ROUND
            uint64_t live;
            MZ_BALLOT(live, !(P(cpos) & 0x1000u));
            MZ_LZ_SELECT_MARK;
            const uint32_t ntok = mz_popc64(live); /* tokens sit in lanes 0..ntok-1 */
            PV(uint32_t, tpk);
            MZ_GATHER4(tpk, pk, P(cpos));
            if (ntok) { /* where the chain left this step: position of the last token + its length */
                const uint32_t lastpos = MZ_READLANE(cpos, ntok - 1u) >> 2;
                const uint32_t lastpk = MZ_READLANE(tpk, ntok - 1u);
                const uint32_t nx = lastpos + ((lastpk & 511u) ? (lastpk & 511u) : 1u);
                skip = nx > 64u ? nx - 64u : 0u;
            } else {
                skip = skip > 64u ? skip - 64u : 0u;
            }
