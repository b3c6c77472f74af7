// emul_bzip2_enc.cpp -- host build of minizip-ng_amd/csrc/bzip2_enc_core.h (g++ -DMZHIP_HOST_EMUL) for
// tests/test_bzip2_enc_emul.py: one "wave" = one LDS block and one scratch, as a resident wave of k_bzip2_encode_batch owns
// them, and entries run through it one after the other, so that whatever an entry leaves behind meets the next.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bzip2_enc_core.h"

#define EMUL_API extern "C" __attribute__((visibility("default")))

struct emul_bze_wave {
    mz_bze_lds lds;
    mzhip_crc_tables tabs;
    uint32_t max_in_len;
    uint8_t *scratch[10]; // per block-size digit, exactly MZ_BZE_SCRATCH_BYTES of the launch: a sanitised build reports the first byte outside
};

// a wave of a launch whose largest entry has max_in_len bytes
EMUL_API emul_bze_wave *emul_bzip2_enc_wave_new(uint32_t max_in_len) {
    emul_bze_wave *w = (emul_bze_wave *)malloc(sizeof(emul_bze_wave));
    memset(&w->lds, 0xA5, sizeof(w->lds)); // nothing may rely on zeroed LDS or scratch
    mzhip_crc_tables_init(&w->tabs);
    w->max_in_len = max_in_len;
    for (int d = 0; d < 10; d++) w->scratch[d] = nullptr;
    return w;
}

EMUL_API void emul_bzip2_enc_wave_free(emul_bze_wave *w) {
    for (int d = 0; d < 10; d++) free(w->scratch[d]);
    free(w);
}

EMUL_API int32_t emul_bzip2_enc_run(emul_bze_wave *w, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, int32_t level,
                                    uint32_t *out_len, uint32_t *crc) {
    const uint32_t digit = MZ_BZE_LEVEL(level);
    if (!digit) return -102;
    const uint32_t cap = MZ_BZE_CAP_SYMS(w->max_in_len, digit);
    if (!w->scratch[digit]) {
        w->scratch[digit] = (uint8_t *)malloc(MZ_BZE_SCRATCH_BYTES(cap));
        memset(w->scratch[digit], 0xA5, MZ_BZE_SCRATCH_BYTES(cap));
    }
    mz_bze_result r;
    mz_bzip2_enc_entry(in, in_len, out, out_cap, digit, cap, &w->lds, w->tabs.byte_tab, &w->tabs, w->scratch[digit], &r);
    *out_len = r.out_len;
    *crc = r.crc;
    return r.status;
}

EMUL_API uint32_t emul_bzip2_enc_lds_bytes(void) { return (uint32_t)sizeof(mz_bze_lds); }
EMUL_API uint64_t emul_bzip2_enc_scratch_bytes(uint32_t max_in_len, int32_t level) {
    return MZ_BZE_SCRATCH_BYTES(MZ_BZE_CAP_SYMS(max_in_len, MZ_BZE_LEVEL(level)));
}
EMUL_API uint64_t emul_bzip2_enc_bound(uint32_t in_len, int32_t level) { // as mzhip_bzip2_encode_bound
    const uint64_t digit = MZ_BZE_LEVEL(level);
    return digit ? MZ_BZE_BOUND(in_len, digit) : 0u;
}

#ifdef EMUL_BZIP2_ENC_MAIN
// stand-alone run for a sanitised host build (-fsanitize=address,undefined): emul_bzip2_enc_san LEVEL FILE [FILE ...] encodes
// every file through ONE wave sized for the largest, input and output in exact-size heap buffers (output: the bound, then
// the size it took, then one byte less), writes FILE.bz2 and prints "status out_len crc status_exact status_short" per file
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int32_t level = (int32_t)strtol(argv[1], nullptr, 10);
    long biggest = 0;
    for (int i = 2; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        if (ftell(f) > biggest) biggest = ftell(f);
        fclose(f);
    }
    emul_bze_wave *w = emul_bzip2_enc_wave_new((uint32_t)biggest);
    for (int i = 2; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *in = (uint8_t *)malloc((size_t)n); // (malloc(0): a valid pointer with no byte behind it)
        if (n > 0 && fread(in, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        const uint32_t cap = (uint32_t)emul_bzip2_enc_bound((uint32_t)n, level);
        uint8_t *out = (uint8_t *)malloc(cap);
        uint32_t ol = 0, crc = 0, ol2 = 0, c2 = 0;
        const int32_t st = emul_bzip2_enc_run(w, in, (uint32_t)n, out, cap, level, &ol, &crc);
        char name[4096];
        snprintf(name, sizeof(name), "%s.bz2", argv[i]);
        FILE *g = fopen(name, "wb");
        if (!g) return 2;
        if (ol) fwrite(out, 1, ol, g);
        fclose(g);
        uint8_t *exact = (uint8_t *)malloc(ol);
        const int32_t st_exact = emul_bzip2_enc_run(w, in, (uint32_t)n, exact, ol, level, &ol2, &c2);
        const int same = st_exact == 0 && ol2 == ol && memcmp(exact, out, ol) == 0;
        free(exact);
        uint8_t *tight = (uint8_t *)malloc(ol ? ol - 1 : 0);
        const int32_t st_short = emul_bzip2_enc_run(w, in, (uint32_t)n, tight, ol ? ol - 1 : 0, level, &ol2, &c2);
        free(tight);
        printf("%d %u %u %d %d\n", st, ol, crc, same ? 0 : -1, st_short);
        free(out);
        free(in);
    }
    emul_bzip2_enc_wave_free(w);
    return 0;
}
#endif
