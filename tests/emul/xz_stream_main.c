/* tests/emul/xz_stream_main.c -- TEST INFRASTRUCTURE.  A program of its own for the sanitizers: mz_stream_lzma READ of method 95
 * (minizip-ng_amd/csrc/shim_lzma.c on the host emulation, tests/emul/libmockdrop.so built with SAN=address) over
 * the frame programs of tests/xz_frames.py.  tests/test_xz_frames.py::test_sanitised_stream_program writes the cases, links
 * this file against that library with the same sanitizer and runs it as a child process; a read or write outside a heap
 * block -- the shim's own input and output buffers among them -- ends it with a report.
 *
 *     xz_stream_main cases.bin      cases.bin: u32 n, then n x { u32 length, u32 out_cap, u32 size of the data or 0xFFFFFFFF, bytes }
 *
 * Every case is read whole and in 7-byte read() calls, without limits and with the ones mz_zip sets.  One line per run:
 *     case chunk limits n_rets last_ret produced total_out close crc32(out)                                              */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int32_t drv_stream_decode(int32_t method, const uint8_t *in, int32_t in_len, int64_t max_in, int64_t max_out, int32_t window_bits,
                          uint8_t *out, int32_t out_cap, int32_t chunk, int32_t *rets, int32_t max_rets, int64_t *info);

static uint32_t crc32_bytes(const uint8_t *p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++)
            c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

int main(int argc, char **argv) {
    enum { MAX_RETS = 4096 };
    static int32_t rets[MAX_RETS];
    if (argc < 2)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    uint32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1)
        return 2;
    for (uint32_t c = 0; c < n; c++) {
        uint32_t h[3];
        if (fread(h, 4, 3, f) != 3)
            return 2;
        uint8_t *in = (uint8_t *)malloc(h[0] ? h[0] : 1); /* a heap block of the stream's exact length */
        uint8_t *out = (uint8_t *)malloc(h[1]);
        if (!in || !out || (h[0] && fread(in, 1, h[0], f) != h[0]))
            return 2;
        for (int chunk = 65535; chunk >= 7; chunk = chunk == 65535 ? 7 : 0) {
            for (int lim = 0; lim < 2; lim++) {
                int64_t info[6];
                if (lim && h[0] == 0)
                    continue;
                memset(out, 0, h[1]);
                const int32_t nr = drv_stream_decode(95, in, (int32_t)h[0], lim ? (int64_t)h[0] : 0,
                                                     lim && h[2] != 0xFFFFFFFFu ? (int64_t)h[2] : -1, 0, out, (int32_t)h[1], chunk, rets,
                                                     MAX_RETS, info);
                int64_t produced = 0;
                for (int32_t i = 0; i < nr && i < MAX_RETS; i++)
                    if (rets[i] > 0)
                        produced += rets[i];
                printf("%u %d %d %d %d %lld %lld %lld %u\n", c, chunk, lim, nr, nr > 0 && nr <= MAX_RETS ? rets[nr - 1] : 0,
                       (long long)produced, (long long)info[1], (long long)info[2], crc32_bytes(out, (size_t)produced));
            }
        }
        free(in);
        free(out);
    }
    fclose(f);
    return 0;
}
