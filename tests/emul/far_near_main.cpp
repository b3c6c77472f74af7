// far_near_main.cpp -- the host emulation of K1 alone, around the far / near lists of its commit (TEST INFRASTRUCTURE;
// inflate_emit.inc classes every piece of a back-reference as far, near or split, inflate_commit.inc copies the far list, then
// the near list).  Two uses of one text:
//   a shared library with -DMZ_STATS (no sanitizer): fn_inflate() decodes one entry between red zones -- in front of and behind
//     the output, the wave's record scratch and its LDS -- and hands back the four result words, the kernel's counters of that
//     one decode, and whether every red zone is intact (tests/far_near_cases.py, tests/test_far_near_lists_emul.py);
//   a program with -fsanitize=address,undefined: every stream of a case file at four output misalignments, from heap blocks
//     that end with the input's last aligned dword and the output's capacity.
//
//     far_near_main <cases>
//
// cases: uint32 n, then n times { uint32 in_len, uint32 out_cap, in_len bytes }.  One line per case and misalignment on
// stdout: case mis status out_len in_used crc.  Exit status 3: a red zone was written.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "inflate_core.h"
#if defined(MZ_STATS)
unsigned long long mz_stats[32], mz_stat_max;
#endif

#define FN_ZONE 256u
static mzhip_crc_tables g_tabs;

static int zone_ok(const uint8_t *p, uint8_t v) {
    for (uint32_t k = 0; k < FN_ZONE; k++)
        if (p[k] != v) return 0;
    return 1;
}

/* one decode; the record scratch and the LDS between red zones of their own.  -> 1 when both pairs of zones are intact */
static int decode(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, mz_inflate_result *r) {
    const size_t lds = (sizeof(mz_inflate_lds) + 15u) & ~(size_t)15u;
    uint8_t *lb = (uint8_t *)malloc(lds + 2u * FN_ZONE);
    uint8_t *rb = (uint8_t *)malloc((size_t)MZ_REC_BYTES + 2u * FN_ZONE);
    memset(lb, 0xA5, lds + 2u * FN_ZONE);
    memset(rb, 0x5A, (size_t)MZ_REC_BYTES + 2u * FN_ZONE);
    mz_inflate_entry(in, in_len, out, out_cap, (mz_inflate_lds *)(lb + FN_ZONE), g_tabs.byte_tab, &g_tabs, 1u, rb + FN_ZONE, (const mz_inflate_state *)0,
                     (mz_inflate_state *)0, r, (const mz_inflate_par *)0);
    const int ok = zone_ok(lb, 0xA5) && zone_ok(lb + FN_ZONE + lds, 0xA5) && zone_ok(rb, 0x5A) && zone_ok(rb + FN_ZONE + MZ_REC_BYTES, 0x5A);
    free(rb);
    free(lb);
    return ok;
}

/* buf: FN_ZONE + omis bytes in front of the output, out_cap bytes of output, FN_ZONE behind, all poisoned by the caller (who
 * checks them); words: status, out_len, in_used, crc; stats: the 32 counters of this decode (zeros without MZ_STATS) */
extern "C" int32_t fn_inflate(const uint8_t *in, uint32_t in_len, uint8_t *buf, uint32_t omis, uint32_t out_cap, uint32_t *words,
                              unsigned long long *stats) {
    static const int once = (mzhip_crc_tables_init(&g_tabs), 1);
    (void)once;
#if defined(MZ_STATS)
    memset(mz_stats, 0, sizeof(mz_stats));
    mz_stat_max = 0;
#endif
    mz_inflate_result r;
    const int ok = decode(in, in_len, buf + FN_ZONE + omis, out_cap, &r);
    words[0] = (uint32_t)r.status;
    words[1] = r.out_len;
    words[2] = r.in_used;
    words[3] = r.crc;
    for (uint32_t k = 0; k < 32u; k++) {
#if defined(MZ_STATS)
        stats[k] = mz_stats[k];
#else
        stats[k] = 0;
#endif
    }
    return ok;
}
extern "C" uint32_t fn_zone(void) { return FN_ZONE; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    mzhip_crc_tables_init(&g_tabs);
    uint32_t n = 0;
    int intact = 1;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < n; c++) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        const uint32_t len = hdr[0], cap = hdr[1];
        uint8_t *z = (uint8_t *)malloc(len ? len : 1);
        if (len && fread(z, 1, len, f) != len) return 2;
        for (uint32_t s = 0; s < 4u; s++) {
            /* malloc() returns 16-byte aligned blocks: the input `mis` bytes off a 16-byte boundary in a block that ends with the
             * aligned dword of its last byte (a decoder may read that dword whole), the output `omis` bytes off in a block that
             * ends with the capacity */
            const uint32_t omis = (5u * s + c) & 15u, mis = (7u * s + 3u * c) & 15u;
            const size_t blk = ((size_t)mis + len + 3u) & ~(size_t)3u;
            uint8_t *block = (uint8_t *)malloc(blk ? blk : 1);
            memset(block, 0xC3, blk);
            memcpy(block + mis, z, len);
            uint8_t *oblk = (uint8_t *)malloc((size_t)omis + cap ? (size_t)omis + cap : 1u);
            mz_inflate_result r;
            intact &= decode(block + mis, len, oblk + omis, cap, &r);
            printf("%u %u %d %u %u %u\n", c, omis, (int)r.status, r.out_len, r.in_used, r.crc);
            free(oblk);
            free(block);
        }
        free(z);
    }
    fclose(f);
    return intact ? 0 : 3;
}
