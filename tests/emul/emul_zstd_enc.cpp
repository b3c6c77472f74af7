// emul_zstd_enc.cpp -- host build of minizip-ng_amd/csrc/zstd_enc_core.h (g++ -DMZHIP_HOST_EMUL) for
// tests/test_zstd_enc_emul.py: the parse of lzma_enc_core.h (the chain pass for an entry of more than one block, then the
// tokenizer block by block, one LDS slice and one xhead) and behind it one "wave" of the coder = one LDS block and one scratch, as a
// resident wave of k_zstd_encode_batch owns them; entries run through it one after the other, so that whatever an entry
// leaves behind meets the next.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "zstd_enc_core.h"

#define EMUL_API extern "C" __attribute__((visibility("default")))

struct emul_zse_wave {
    mz_zse_lds lds;
    mz_lz_tok_lds tok_lds;
    mzhip_crc_tables tabs;
    uint16_t *xhead;
    uint32_t *chain_head;
    uint8_t *scratch; // exactly MZ_ZSE_SCRATCH_BYTES: a sanitised build reports the first byte outside
};

EMUL_API emul_zse_wave *emul_zstd_enc_wave_new(void) {
    emul_zse_wave *w = (emul_zse_wave *)malloc(sizeof(emul_zse_wave));
    const size_t xbytes = (MZ_DEF_WAYS_BEST - 1u) * (sizeof(uint16_t) << MZ_DEF_HBITS);
    memset(&w->lds, 0xA5, sizeof(w->lds)); // nothing may rely on zeroed LDS or scratch
    memset(&w->tok_lds, 0xA5, sizeof(w->tok_lds));
    mzhip_crc_tables_init(&w->tabs);
    w->xhead = (uint16_t *)malloc(xbytes);
    memset(w->xhead, 0xA5, xbytes);
    w->chain_head = (uint32_t *)malloc(sizeof(uint32_t) << MZ_LZE_FAR_HBITS);
    memset(w->chain_head, 0xA5, sizeof(uint32_t) << MZ_LZE_FAR_HBITS);
    w->scratch = (uint8_t *)malloc(MZ_ZSE_SCRATCH_BYTES);
    memset(w->scratch, 0xA5, MZ_ZSE_SCRATCH_BYTES);
    return w;
}

EMUL_API void emul_zstd_enc_wave_free(emul_zse_wave *w) {
    free(w->xhead);
    free(w->chain_head);
    free(w->scratch);
    free(w);
}

// level as mzhip_zstd_encode_batch takes it; flags bit 0 = content checksum
EMUL_API int32_t emul_zstd_enc_run(emul_zse_wave *w, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, int32_t level,
                                   uint32_t flags, uint32_t *out_len, uint32_t *crc) {
    if (!MZ_ZSE_LEVEL_OK(level)) return -102;
    const int32_t preset = MZ_ZSE_PRESET(level);
    const uint32_t ways = (preset >= 0 && preset <= 3) ? 1u : MZ_DEF_WAYS_BEST, far_depth = MZ_LZE_DEPTH_FOR_PRESET(preset);
    const uint32_t nblocks = (in_len + MZ_DEF_BLOCK - 1) / MZ_DEF_BLOCK;
    const size_t words = (size_t)(nblocks ? nblocks : 1) * MZ_DEF_BLOCK;
    uint32_t *tok = (uint32_t *)malloc(words * sizeof(uint32_t));
    uint32_t *ntok = (uint32_t *)calloc(nblocks ? nblocks : 1, sizeof(uint32_t));
    uint32_t *links = nullptr;
    memset(tok, 0xA5, words * sizeof(uint32_t));
    if (in_len > MZ_DEF_BLOCK) { // the chain pass (k_lz_chain_batch): one wave over the whole entry
        links = (uint32_t *)malloc(words * sizeof(uint32_t));
        memset(links, 0xA5, words * sizeof(uint32_t));
        mz_lz_chain(in, in_len, links, w->chain_head);
    }
    for (uint32_t b = 0; b < nblocks; b++) {
        const uint32_t lo = b * MZ_DEF_BLOCK, hi = (in_len - lo < MZ_DEF_BLOCK) ? in_len : lo + MZ_DEF_BLOCK;
        ntok[b] = mz_lz_tokenize(in, lo, hi, tok + (size_t)b * MZ_DEF_BLOCK, &w->tok_lds, ways, ways > 1u ? w->xhead : (uint16_t *)0, links, far_depth);
    }
    mz_zse_result r;
    mz_zstd_enc_entry(in, in_len, tok, ntok, out, out_cap, flags, &w->lds, w->tabs.byte_tab, &w->tabs, w->scratch, &r);
    free(links);
    free(ntok);
    free(tok);
    *out_len = r.out_len;
    *crc = r.crc;
    return r.status;
}

EMUL_API uint32_t emul_zstd_enc_lds_bytes(void) { return (uint32_t)sizeof(mz_zse_lds); }
EMUL_API uint32_t emul_zstd_enc_scratch_bytes(void) { return MZ_ZSE_SCRATCH_BYTES; }
EMUL_API uint64_t emul_zstd_enc_bound(uint32_t in_len) { return MZ_ZSE_BOUND(in_len); } // as mzhip_zstd_encode_bound
// the most sequences any block had since the last reset
EMUL_API uint32_t emul_zstd_enc_max_nseq(int reset) {
    const uint32_t v = mz_zse_max_nseq;
    if (reset) mz_zse_max_nseq = 0;
    return v;
}

#ifdef EMUL_ZSTD_ENC_MAIN
// stand-alone run for a sanitised host build (-fsanitize=address,undefined): emul_zstd_enc_san LEVEL FLAGS FILE [FILE ...]
// encodes every file through ONE wave, input and output in exact-size heap buffers (output: the bound, then the size it
// took, then one byte less), writes FILE.zst and prints "status out_len crc status_exact status_short" per file
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const int32_t level = (int32_t)strtol(argv[1], nullptr, 10);
    const uint32_t flags = (uint32_t)strtoul(argv[2], nullptr, 10);
    emul_zse_wave *w = emul_zstd_enc_wave_new();
    for (int i = 3; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *in = (uint8_t *)malloc((size_t)n); // (malloc(0): a valid pointer with no byte behind it)
        if (n > 0 && fread(in, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        const uint32_t cap = (uint32_t)emul_zstd_enc_bound((uint32_t)n);
        uint8_t *out = (uint8_t *)malloc(cap);
        uint32_t ol = 0, crc = 0, ol2 = 0, c2 = 0;
        const int32_t st = emul_zstd_enc_run(w, in, (uint32_t)n, out, cap, level, flags, &ol, &crc);
        char name[4096];
        snprintf(name, sizeof(name), "%s.zst", argv[i]);
        FILE *g = fopen(name, "wb");
        if (!g) return 2;
        if (ol) fwrite(out, 1, ol, g);
        fclose(g);
        uint8_t *exact = (uint8_t *)malloc(ol);
        const int32_t st_exact = emul_zstd_enc_run(w, in, (uint32_t)n, exact, ol, level, flags, &ol2, &c2);
        const int same = st_exact == 0 && ol2 == ol && memcmp(exact, out, ol) == 0;
        free(exact);
        uint8_t *tight = (uint8_t *)malloc(ol ? ol - 1 : 0);
        const int32_t st_short = emul_zstd_enc_run(w, in, (uint32_t)n, tight, ol ? ol - 1 : 0, level, flags, &ol2, &c2);
        free(tight);
        printf("%d %u %u %d %d\n", st, ol, crc, same ? 0 : -1, st_short);
        free(out);
        free(in);
    }
    emul_zstd_enc_wave_free(w);
    return 0;
}
#endif
