// emul_zstd_large.cpp -- host build of minizip-ng_amd/csrc/zstd_par_core.h (g++ -DMZHIP_HOST_EMUL) behind the host logic of
// zstd_parallel.inc, for tests/test_zstd_large_emul.py: what mzhip_zstd_large does on the device, with loops over the 64-lane
// emulation in place of kernel launches.  The blocks of a pass run in a SHUFFLED order, every one through LDS and scratch
// filled with a pattern, so a hidden dependence on order or on what another block left behind shows.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zstd_par_core.h"
#include "zstd_parallel.inc"

#define EMUL_API extern "C" __attribute__((visibility("default")))

namespace {
struct EmulBackend {
    const uint8_t *in;
    uint32_t in_len;
    uint8_t *out;
    uint32_t *map; // exactly map_n words: a sanitised build reports the first one outside
    uint32_t map_n, seed;
    mz_zs_lds lds;
    uint8_t *scratch;
    int32_t scan(uint32_t blk_cap, std::vector<uint32_t> &recs, std::vector<uint32_t> &frms, uint32_t *hdr) {
        recs.assign((size_t)blk_cap * MZ_ZSP_REC_WORDS, 0xA5A5A5A5u);
        frms.assign(((size_t)blk_cap + 1u) * MZ_ZSP_FRM_WORDS, 0xA5A5A5A5u);
        memset(&lds, 0xA5, sizeof(lds));
        mz_zsp_scan(in, in_len, &lds, recs.data(), frms.data(), blk_cap, hdr);
        return 0;
    }
    int32_t blocks(uint32_t mode, const uint32_t *jobs, uint32_t n, uint32_t bias, uint32_t *res) {
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        for (uint32_t i = n; i > 1u; i--) {
            seed = seed * 1664525u + 1013904223u;
            std::swap(order[i - 1u], order[(seed >> 8) % i]);
        }
        uint32_t *const ptr = (uint32_t *)((uintptr_t)map - 4u * (uintptr_t)bias);
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t e = order[k];
            memset(&lds, 0xA5, sizeof(lds));
            memset(scratch, 0xA5, MZ_ZS_SCRATCH_BYTES);
            if (mode == 2u && jobs[(size_t)e * MZ_ZSP_JOB_WORDS + MZ_ZSP_J_END] - bias > map_n) return -104;
            mz_zsp_block(in, in_len, jobs + (size_t)e * MZ_ZSP_JOB_WORDS, mode, out, ptr, &lds, scratch, res + (size_t)e * MZ_ZSP_RES_WORDS);
        }
        return 0;
    }
    // the device's rounds: up to four links per position and round, two rounds per look at the flag
    int32_t resolve(uint32_t w0, uint32_t w1, uint32_t *rounds) {
        uint32_t *const ptr = (uint32_t *)((uintptr_t)map - 4u * (uintptr_t)w0);
        if (w1 - w0 > map_n) return -104;
        for (uint32_t r = 0; r < 40u; r++) {
            uint32_t changed = 0;
            for (uint32_t half = 0; half < 2u; half++)
                for (uint64_t i = w0; i < w1; i++) {
                    uint32_t p = ptr[i], moved = 0;
                    if (p == (uint32_t)i || p < w0) continue;
                    if (p >= w1) return -104;
                    for (int k = 0; k < 4; k++) {
                        const uint32_t q = ptr[p];
                        if (q == p) break;
                        p = q;
                        moved = 1;
                        if (p < w0) break;
                    }
                    if (moved) {
                        ptr[i] = p;
                        changed = 1;
                    }
                }
            *rounds += 2;
            if (!changed) break;
        }
        for (uint64_t i = w0; i < w1; i++)
            if (ptr[i] != (uint32_t)i) out[i] = out[ptr[i]];
        return 0;
    }
    int32_t xxh(const uint32_t *spans, uint32_t n, uint32_t *vals) {
        for (uint32_t k = 0; k < n; k++) vals[k] = mz_zsp_xxh64(out + spans[2u * k], spans[2u * k + 1u]);
        return 0;
    }
};
} // namespace

// the one-wave reader of zstd_core.h: what every field is compared with
EMUL_API int32_t emul_zstd_one(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len, uint32_t *in_used,
                               uint32_t *crc) {
    mz_zs_lds *lds = (mz_zs_lds *)malloc(sizeof(mz_zs_lds));
    uint8_t *scratch = (uint8_t *)malloc(MZ_ZS_SCRATCH_BYTES);
    mzhip_crc_tables tabs;
    mz_zs_result r;
    memset(lds, 0xA5, sizeof(*lds));
    memset(scratch, 0xA5, MZ_ZS_SCRATCH_BYTES);
    mzhip_crc_tables_init(&tabs);
    mz_zstd_entry(in, in_len, out, out_cap, lds, tabs.byte_tab, &tabs, scratch, &r);
    free(scratch);
    free(lds);
    *out_len = r.out_len;
    *in_used = r.in_used;
    *crc = r.crc;
    return r.status;
}

// mzhip_zstd_large on the host: stats[0 .. 6) in the order of mzhip_zstd_large_stats (size, windows, blocks, borrowed, rounds, fallback)
EMUL_API int32_t emul_zstd_large(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t window, uint32_t seed,
                                 uint32_t *out_len, uint32_t *in_used, uint32_t *crc, uint32_t *stats) {
    EmulBackend *be = new EmulBackend;
    MzZsLarge r;
    if (window == 0) window = 128u << 20;
    be->in = in;
    be->in_len = in_len;
    be->out = out;
    be->map_n = window > MZ_ZS_BLOCK_MAX ? window : MZ_ZS_BLOCK_MAX;
    if (be->map_n > out_cap) be->map_n = out_cap;
    be->map = (uint32_t *)malloc((size_t)be->map_n * 4u + 1u);
    memset(be->map, 0xA5, (size_t)be->map_n * 4u);
    be->seed = seed;
    be->scratch = (uint8_t *)malloc(MZ_ZS_SCRATCH_BYTES);
    int32_t st = mz_zstd_large_entry(*be, in_len, out_cap, window, &r);
    free(be->scratch);
    free(be->map);
    delete be;
    if (st != 0) r.fallback = 3u;
    stats[0] = 24u;
    stats[1] = r.windows;
    stats[2] = r.blocks;
    stats[3] = r.borrowed;
    stats[4] = r.rounds;
    stats[5] = r.fallback;
    if (r.fallback) return emul_zstd_one(in, in_len, out, out_cap, out_len, in_used, crc);
    {
        mzhip_crc_tables tabs;
        uint32_t c = 0xFFFFFFFFu;
        mzhip_crc_tables_init(&tabs);
        for (uint32_t i = 0; i < r.out_len; i++) c = tabs.byte_tab[(c ^ out[i]) & 255u] ^ (c >> 8);
        *crc = ~c;
    }
    *out_len = r.out_len;
    *in_used = in_len;
    return 0;
}

EMUL_API uint32_t emul_zstd_large_xxh64_low(const uint8_t *d, uint32_t n) { return mz_zsp_xxh64(d, n); }

#ifdef EMUL_ZSTD_LARGE_MAIN
// stand-alone run for a sanitised host build (-fsanitize=address,undefined): emul_zstd_large_san FILE CAP WINDOW [...] decodes
// every file, input and output in exact-size heap buffers, and prints "status out_len in_used crc fallback blocks" per file
#include <stdio.h>
int main(int argc, char **argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *exact = (uint8_t *)malloc((size_t)n);
        if (n > 0 && fread(exact, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        const uint32_t cap = (uint32_t)strtoul(argv[i + 1], nullptr, 10), window = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
        uint8_t *out = (uint8_t *)malloc(cap);
        uint32_t ol = 0, iu = 0, crc = 0, stats[6] = {0};
        const int32_t st = emul_zstd_large(exact, (uint32_t)n, out, cap, window, (uint32_t)i, &ol, &iu, &crc, stats);
        printf("%d %u %u %u %u %u\n", st, ol, iu, crc, stats[5], stats[2]);
        free(out);
        free(exact);
    }
    return 0;
}
#endif
