/* deflate_select.inc -- K4, one step of 64 positions: the shared selection (lz77_select.inc, which names what it expects
 * and leaves), then what DEFLATE does with the step's tokens.  Textually included by mz_deflate_piece() (deflate_core.h)
 * -- in pass 1 behind the lazy rule, and again behind the cost parse.  The tokens are appended to tok[] where
 * MZ_DEF_STORE_TOKENS; the histograms, xbits and ntokens are updated. */
#define MZ_LZ_SELECT_MARK MZ_DPROF_MARK(19) /* lazy rule + greedy selection */
#include "lz77_select.inc"
#undef MZ_LZ_SELECT_MARK
            MZ_LANES {
                if ((uint32_t)lane < ntok) {
                    const uint32_t t = P(tpk), mlen = t & 511u;
                    if (MZ_DEF_STORE_TOKENS) tok[ntokens + (uint32_t)lane] = t;
                    if (mlen == 0u) {
                        MZ_LDS_ATOMIC_INC(&L->freq[t >> 9]);
                    } else {
                        uint32_t ex, xv, dx;
                        MZ_LDS_ATOMIC_INC(&L->freq[mz_len_sym(mlen, &ex, &xv)]);
                        MZ_LDS_ATOMIC_INC(&L->freq[MZ_DEF_DIST0 + mz_dist_sym(t >> 9, &dx, &xv)]);
                        P(xbits) += ex + dx;
                    }
                }
            }
            ntokens += ntok;
