// emul_bzip2.cpp -- host build of minizip-ng_amd/csrc/bzip2_core.h (g++ -DMZHIP_HOST_EMUL) for tests/test_bzip2_emul.py:
// one "wave" = one LDS block and one scratch, as a resident wave of k_bzip2_batch owns them, and entries run through it
// one after the other, so that whatever an entry leaves behind meets the next.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bzip2_core.h"

#define EMUL_API extern "C" __attribute__((visibility("default")))

struct emul_bz_wave {
    mz_bz_lds lds;
    mzhip_crc_tables tabs;
    uint8_t *scratch; // exactly MZ_BZ_SCRATCH_BYTES: a sanitised build reports the first byte outside
};

EMUL_API emul_bz_wave *emul_bzip2_wave_new(void) {
    emul_bz_wave *w = (emul_bz_wave *)malloc(sizeof(emul_bz_wave));
    memset(&w->lds, 0xA5, sizeof(w->lds)); // nothing may rely on zeroed LDS or scratch
    mzhip_crc_tables_init(&w->tabs);
    w->scratch = (uint8_t *)malloc(MZ_BZ_SCRATCH_BYTES);
    memset(w->scratch, 0xA5, MZ_BZ_SCRATCH_BYTES);
    return w;
}

EMUL_API void emul_bzip2_wave_free(emul_bz_wave *w) {
    free(w->scratch);
    free(w);
}

EMUL_API int32_t emul_bzip2_run(emul_bz_wave *w, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len,
                                uint32_t *in_used, uint32_t *crc) {
    mz_bz_result r;
    mz_bzip2_entry(in, in_len, out, out_cap, &w->lds, w->tabs.byte_tab, &w->tabs, w->scratch, &r);
    *out_len = r.out_len;
    *in_used = r.in_used;
    *crc = r.crc;
    return r.status;
}

EMUL_API uint32_t emul_bzip2_lds_bytes(void) { return (uint32_t)sizeof(mz_bz_lds); }
EMUL_API uint32_t emul_bzip2_scratch_bytes(void) { return MZ_BZ_SCRATCH_BYTES; }

#ifdef EMUL_BZIP2_MAIN
// stand-alone run for a sanitised host build (-fsanitize=address,undefined): emul_bzip2_san FILE CAP [FILE CAP ...] decodes
// every file through ONE wave, input and output in exact-size heap buffers, and prints "status out_len in_used crc" per file
#include <stdio.h>
int main(int argc, char **argv) {
    emul_bz_wave *w = emul_bzip2_wave_new();
    for (int i = 1; i + 1 < argc; i += 2) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *in = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0 && fread(in, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        uint8_t *exact = (uint8_t *)malloc((size_t)n); // (malloc(0): a valid pointer with no byte behind it)
        memcpy(exact, in, (size_t)n);
        const uint32_t cap = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
        uint8_t *out = (uint8_t *)malloc(cap);
        uint32_t ol = 0, iu = 0, crc = 0;
        const int32_t st = emul_bzip2_run(w, exact, (uint32_t)n, out, cap, &ol, &iu, &crc);
        printf("%d %u %u %u\n", st, ol, iu, crc);
        free(out);
        free(exact);
        free(in);
    }
    emul_bzip2_wave_free(w);
    return 0;
}
#endif
