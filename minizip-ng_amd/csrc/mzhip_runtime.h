// mzhip_runtime.h -- the seam between the two halves of libmzhip.so's C++ runtime.  PRIVATE: not part of the ABI, every
// name here has hidden visibility.
//   device TU  mzhip_kernels.hip + mzhip_launch.inc (hipcc): the kernels and every function whose body names a kernel, a
//              kernel argument struct or a constant of a core header -- device context, launchers -- and the one definition of
//              the scratch and work-queue caches (mzhip_slots.inc, whose declarations both halves see: the leases below);
//   host TUs   mzhip_host.cpp, mzhip_crc_host.cpp, mzhip_prime.cpp (the host C++ compiler, <hip/hip_runtime_api.h> only):
//              device queries, the per-thread stream pool, staging, the one-entry host calls that only call launchers, the
//              CRC lane, the RCCL gather, both prime caches.
// This header declares exactly what crosses between them and names no kernel and no core type.  It also carries what both
// halves' one-entry host calls are built on, on the runtime API alone: the copies on a stream, Staging, and HostCall -- the
// context, the staging lease, the carving of the buffer and the meta block's upload and fetch of one such call.
#ifndef MZHIP_RUNTIME_H
#define MZHIP_RUNTIME_H

#include <hip/hip_runtime_api.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mzhip.h"

#include "mzhip_slots.inc"

namespace mzh {

// ---- defined in mzhip_host.cpp
extern __thread char g_err[256]; // the text behind mzhip_last_error(), per thread
int32_t fail(const char *what, hipError_t e);
#define HIP_TRY(expr)                               \
    do {                                            \
        hipError_t _e = (expr);                     \
        if (_e != hipSuccess) return mzh::fail(#expr, _e); \
    } while (0)

// the calling thread's own non-blocking stream on the current device (made on first use, recycled when the thread exits)
hipStream_t mz_host_stream();
#define MZ_HOST_STREAM mzh::mz_host_stream()

// ---- defined in mzhip_launch.inc
struct DeviceCtx; // per-device state of the launchers: opaque on the host side
constexpr int kMaxDevices = 16;
int32_t ctx_for_current(DeviceCtx **out);
int ctx_device(const DeviceCtx *c); // the device index `c` belongs to
struct ScratchCache;
ScratchCache *ctx_scratch(DeviceCtx *c); // the device's cache of scratch buffers: what a ScratchLease (mzhip_slots.inc) is taken from
// mzhip_deflate_batch_level with `d_warm`: bytes in front of each piece that are hashed as history, not coded (or null)
int32_t deflate_batch_launch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_warm, void *d_out,
                             const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_final, uint32_t n, int32_t level,
                             int32_t window_log2, uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status, void *stream);
// CRC-32 folded on the host with the product's slicing-by-4 tables (the tables are a core header's)
uint32_t crc32_fold_host(uint32_t value, const uint8_t *p, size_t n);
// checksums only: crc(A||B) from crc(A), crc(B), |B|
uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* How the WRITE paths (mz_stream_zlib WRITE's segments, mzhip_prime_write's entries) cut ONE stream for the device: pieces of
 * 16 KiB, a wave each, every piece but the stream's first with the 32 KiB in front of it as history (hashed, not coded:
 * mz_deflate_piece's `warm`).  Up to round 6 the pieces were 64 KiB and blind to each other: a 64 KiB entry was ONE wave's 1 024
 * dependent steps (1.8 ms at level 1; the reference's deflate: 0.5), and matches ended at every cut.  Four times the waves,
 * and the ratio is better than before (text, level 1: 0.3349 against 0.3387; 0.3548 without the history). */
static inline uint32_t def_stream_piece(uint64_t stream_len, int32_t level) {
    /* (the fast class on a short stream -- one 64 KiB entry through the unmodified writer -- is all latency: 8 waves instead of 4;
     * 0.7 % more bytes than 16 KiB pieces on text, still fewer than the 64 KiB pieces of round 5) */
    return (level >= 0 && level <= 3 && stream_len <= (256u << 10)) ? (8u << 10) : (16u << 10);
}
static inline uint32_t def_stream_warm(uint64_t piece_off) { return (uint32_t)(piece_off < 32768u ? piece_off : 32768u) & ~63u; }

// ---- copies on a stream, and the staging of the synchronous host-buffer calls (both sides use them)
static inline hipError_t mz_h2d_on(hipStream_t s, void *dst, const void *src, size_t n) {
    return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s);
}
static inline hipError_t mz_d2h_on(hipStream_t s, void *dst, const void *src, size_t n) {
    const hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}
static inline hipError_t mz_h2d(void *dst, const void *src, size_t n) {
    return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, MZ_HOST_STREAM); // (pageable source: staged before the call returns)
}
static inline hipError_t mz_d2h(void *dst, const void *src, size_t n) {
    const hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, MZ_HOST_STREAM);
    return e != hipSuccess ? e : hipStreamSynchronize(MZ_HOST_STREAM);
}
// Staging of the synchronous host-buffer calls: a buffer of the scratch cache instead of a hipMalloc / hipFree pair
// per call (hipFree alone is a device-wide synchronisation); released when the call returns, after its own sync.
struct Staging : ScratchLease {
    int32_t get(DeviceCtx *ctx, size_t bytes) { return ScratchLease::get(ctx_scratch(ctx), bytes, MZ_HOST_STREAM); }
};

// The round trip of a synchronous one-entry host call, once: the device context, the staging lease, the carving of the
// buffer and the traffic of the call's meta block (the words a batch of one reads and writes: offsets, lengths, status,
// states -- whatever the call's `Meta` holds; it lies first in the buffer).  A call states its layout as take() steps before
// begin() and asks at() for the regions' addresses after it; offsets are from the buffer's first byte, which is what the
// batch launchers' in_off / out_off count from as well.
struct StagedCall {
    DeviceCtx *c = nullptr;
    size_t take(size_t bytes, size_t align = 16) { // the next region: `bytes` at a multiple of `align` -> its offset
        const size_t off = (end + align - 1) & ~(align - 1);
        end = off + bytes;
        return off;
    }
    int32_t begin() { // everything is taken: the context of the current device (unless the call has set `c`) and a staging buffer that holds it all
        const int32_t rc = c ? 0 : ctx_for_current(&c);
        return rc ? rc : sc.get(c, end);
    }
    uint8_t *at(size_t off) const { return (uint8_t *)sc.p + off; }

  private:
    Staging sc;
    size_t end = 0;
};
template <class Meta>
struct HostCall : StagedCall {
    Meta m;             // the host's copy, zeroed
    Meta *dm = nullptr; // the device's (after begin)
    HostCall() {
        memset(&m, 0, sizeof(m));
        take(sizeof(Meta), 64);
    }
    int32_t begin() {
        const int32_t rc = StagedCall::begin();
        dm = (Meta *)at(0);
        return rc;
    }
    hipError_t put_meta() { return mz_h2d(dm, &m, sizeof(m)); }
    hipError_t fetch_meta() { return mz_d2h(&m, dm, sizeof(m)); } // the copy behind the launches, and the wait for it
    hipError_t wait_fetch_meta() {                                // the stream's wait of its own first, where a call has always had one
        const hipError_t e = hipStreamSynchronize(MZ_HOST_STREAM);
        return e != hipSuccess ? e : fetch_meta();
    }
};
// a result the caller may not have asked for: a null pointer is skipped
template <class T, class V>
static inline void give(T *dst, V v) {
    if (dst) *dst = (T)v;
}
// (the .xz container's integers)
static inline void put_le32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// ---- defined in mzhip_host.cpp: checksums of the new bytes of a decoded window (the many-wave decoders of the device TU ask them too)
int32_t window_piece_crcs(uint8_t *base, size_t out_off, uint32_t hist, uint32_t out_len, uint32_t seg_first, uint32_t seg_stride,
                          uint32_t *seg_crc, uint32_t seg_cap, uint32_t *nseg, uint8_t *sm, size_t seg_max);
int32_t window_checksums(uint8_t *base, size_t out_off, uint32_t hist, uint32_t out_len, uint32_t *crc, uint32_t *adler, uint8_t *sm,
                         size_t room, hipStream_t st = nullptr);

} // namespace mzh

// adler(A||B) from those of A and B and |B| (mzhip_launch.inc; shared with the C shims, shim_common.h)
extern "C" uint32_t mzhip_adler32_combine(uint32_t ad_a, uint32_t ad_b, uint64_t len_b);

#endif
