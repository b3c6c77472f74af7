// k1_walk_main.cpp -- a stand-alone program around the host emulation of K1 (TEST INFRASTRUCTURE): decodes every stream of a
// case file from a heap block that ENDS where the input's last aligned dword ends, into a heap block that ends with the
// output's capacity, in one of two sweeps of sixteen decodes per case:
//     in    the input pointer at every misalignment 0 .. 15, the output block as malloc() returns it;
//     out   the output pointer at every misalignment 0 .. 15 and the input pointer at another one each time.
// tests/test_walk_refill_emul.py ("in") and tests/test_chase_lean_emul.py ("out") compile it with -fsanitize=address,undefined
// and run it as a child process: a refill of the walks (inflate_walk.inc) that reads one byte behind what include/mzhip.h lets
// a decoder read, a chase that reads a length or a record outside the wave's record scratch, a rank search that gathers from
// a lane that is none, or a near copy that leaves the staging area is then an error report of the sanitizer, and the program
// ends with its status.  Compiled as a shared library (no sanitizer) it is the emulation of K1 alone: emul_inflate.
//
//     k1_walk_main in|out <cases>
//
// cases: uint32 n, then n times { uint32 in_len, uint32 out_cap, in_len bytes }.  One line per case and misalignment of the
// sweep on stdout: case mis status out_len in_used crc.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "inflate_core.h"

static mzhip_crc_tables g_tabs;

static void decode(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, mz_inflate_result *r) {
    mz_inflate_lds *L = (mz_inflate_lds *)malloc(sizeof(mz_inflate_lds));
    memset(L, 0xA5, sizeof(*L));
    uint8_t *rec = (uint8_t *)malloc(MZ_REC_BYTES);
    memset(rec, 0x5A, MZ_REC_BYTES);
    mz_inflate_entry(in, in_len, out, out_cap, L, g_tabs.byte_tab, &g_tabs, 1u, rec, (const mz_inflate_state *)0, (mz_inflate_state *)0, r,
                     (const mz_inflate_par *)0);
    free(rec);
    free(L);
}

/* the same decode as a library call (tests/emul/emul.cpp emul_inflate, without the other cores) */
extern "C" int32_t emul_inflate(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len, uint32_t *in_used,
                                uint32_t *crc) {
    static const int once = (mzhip_crc_tables_init(&g_tabs), 1);
    (void)once;
    mz_inflate_result r;
    decode(in, in_len, out, out_cap, &r);
    *out_len = r.out_len;
    *in_used = r.in_used;
    *crc = r.crc;
    return r.status;
}

int main(int argc, char **argv) {
    if (argc < 3 || (strcmp(argv[1], "in") != 0 && strcmp(argv[1], "out") != 0)) return 2;
    const int sweep_out = strcmp(argv[1], "out") == 0;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    mzhip_crc_tables_init(&g_tabs);
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < n; c++) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        const uint32_t len = hdr[0], cap = hdr[1];
        uint8_t *z = (uint8_t *)malloc(len ? len : 1);
        if (len && fread(z, 1, len, f) != len) return 2;
        for (uint32_t s = 0; s < 16u; s++) {
            /* malloc() returns 16-byte aligned blocks.  The input: `mis` bytes off a 16-byte boundary, its block ends with the
             * aligned dword that holds the input's last byte (a decoder may read that dword whole: mz_load_stream_dword; where
             * mis + len is a multiple of 4 that is the input's last byte).  The output: `omis` bytes off, its block ends with
             * the capacity. */
            const uint32_t mis = sweep_out ? (s * 5u + c) & 15u : s, omis = sweep_out ? s : 0u;
            const size_t blk = ((size_t)mis + len + 3u) & ~(size_t)3u;
            uint8_t *block = (uint8_t *)malloc(blk ? blk : 1);
            memset(block, 0xC3, blk);
            memcpy(block + mis, z, len);
            uint8_t *oblk = (uint8_t *)malloc((size_t)omis + cap ? (size_t)omis + cap : 1u);
            mz_inflate_result r;
            decode(block + mis, len, oblk + omis, cap, &r);
            printf("%u %u %d %u %u %u\n", c, s, (int)r.status, r.out_len, r.in_used, r.crc);
            free(oblk);
            free(block);
        }
        free(z);
    }
    fclose(f);
    return 0;
}
