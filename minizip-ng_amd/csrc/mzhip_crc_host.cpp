// mzhip_crc_host.cpp -- the host side of mz_crypt_crc32_update: the per-thread page-locked CRC lane, the general staged path,
// fault counting.  It launches through the public mzhip_crc32_batch only.
#include "mzhip_runtime.h"

#include <atomic>
#include <mutex>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace mzh;

extern "C" {

// Host side of mz_crypt_crc32_update.  Buffers below MZHIP_CRC_HOST_BELOW bytes are folded right here with the
// product's own slicing-by-4 tables (the same mzhip_crc_tables the kernels use): a launch plus two PCIe round trips for
// a few bytes helps nobody, and the reference calls this symbol one byte at a time from mz_strm_pkcrypt.c:79,86.
// Larger buffers go to K2 on the device.  The symbol has no error channel (mz_crypt.h:20), so a device failure neither
// aborts the host process nor corrupts the value: the bytes are folded on the host, and the failure is latched for the
// next codec-stream call of this thread to report (mzhip_take_crc_fault, checked by the READ / WRITE shims).
namespace {
thread_local int32_t g_crc_fault = 0;
std::atomic<uint64_t> g_crc_faults{0}; // process-wide, since the start (mzhip_crc_faults)
// A device failure under mz_crypt_crc32_update: the symbol cannot fail (mz_crypt.h:20 returns the checksum), so the value comes
// from this library's own host fold -- and the failure is made as loud as the symbol allows: mzhip_last_error() of the thread
// names it, mzhip_crc_faults() counts it, the thread's next codec-stream call fails with MZ_STREAM_ERROR, and the first one of
// the process says so on stderr ("degrades silently").
void crc_fault(const char *why) {
    char prev[200];
    snprintf(prev, sizeof(prev), "%s", g_err);
    snprintf(g_err, sizeof(g_err), "mz_crypt_crc32_update: device failure (%s%s%s); the checksum was folded on the host", why, prev[0] ? ": " : "", prev);
    g_crc_fault = -1; /* MZ_STREAM_ERROR */
    if (g_crc_faults.fetch_add(1, std::memory_order_relaxed) == 0 && !getenv("MZHIP_QUIET"))
        fprintf(stderr, "mzhip: %s\n", g_err);
}
// MZHIP_FAULT_INJECT=crc (tests): the next device checksum of the process fails as if the device had
bool crc_fault_injected() {
    static std::atomic<int> armed{-1};
    int a = armed.load(std::memory_order_relaxed);
    if (a < 0) {
        const char *e = getenv("MZHIP_FAULT_INJECT");
        a = (e && strcmp(e, "crc") == 0) ? 1 : 0;
        armed.store(a, std::memory_order_relaxed);
    }
    if (a != 1) return false;
    int one = 1;
    return armed.compare_exchange_strong(one, 0);
}
} // namespace

uint64_t mzhip_crc_faults(void) { return g_crc_faults.load(std::memory_order_relaxed); }

namespace {
// mz_crypt_crc32_update is called once per read() / write() of the zip layer (mz_zip.c:2031-2068: 64 KiB at a time from the
// reader and writer loops of mz_zip_rw.c): what a call costs is a launch and its round trips, not the fold.  A call of up to
// 1 MiB goes through a page-locked block of the calling thread: [256 results | 256 offsets | 256 lengths | the bytes], the
// bytes are cut into 4 KiB pieces, a wave each, and the kernel reads them and writes its results in place over the link (no
// copy is queued: one launch, one wait).  Before round 6 the call staged pageable memory into the scratch cache: 119 us per
// 64 KiB (0.51 GiB/s -- 92 % of the 2.1 s a 1 GiB entry took to WRITE through the drop-in, profiles/r6/crc_calls.log).
constexpr size_t kCrcLaneSegs = 256, kCrcLaneHead = kCrcLaneSegs * 16, kCrcLaneData = (size_t)1 << 20, kCrcLanePiece = 4096;
struct CrcLane {
    uint8_t *host = nullptr, *dev = nullptr; // the same block, as the host and as the device address it
    int device = -1;
};
struct CrcLanePool {
    std::mutex mu;
    std::vector<CrcLane> idle;
};
CrcLanePool *crc_lane_pool() {
    static CrcLanePool *p = new CrcLanePool(); // (never deleted: thread_local destructors may run after static ones)
    return p;
}
struct ThreadCrcLane {
    CrcLane lane;
    ~ThreadCrcLane() {
        if (!lane.host) return;
        CrcLanePool *p = crc_lane_pool();
        std::lock_guard<std::mutex> g(p->mu);
        p->idle.push_back(lane); // (handed on to the next thread, never freed: a process has as many as it ever had threads at once)
    }
};
thread_local ThreadCrcLane t_crc_lane;
int crc_lane_mode() { // 2: the kernel reads the block over the link; 1: the block is copied to the device first; 0: the path of rounds 1 - 5
    static const int m = [] {
        const char *e = getenv("MZHIP_CRC_LANE");
        return e && e[0] >= '0' && e[0] <= '2' ? e[0] - '0' : 2;
    }();
    return m;
}
CrcLane *crc_lane_for(int device) {
    CrcLane &l = t_crc_lane.lane;
    if (l.host && l.device == device) return &l;
    if (l.host) { // (the thread moved to another device: the block it has goes back)
        CrcLanePool *p = crc_lane_pool();
        std::lock_guard<std::mutex> g(p->mu);
        p->idle.push_back(l);
        l = CrcLane();
    }
    {
        CrcLanePool *p = crc_lane_pool();
        std::lock_guard<std::mutex> g(p->mu);
        for (size_t i = 0; i < p->idle.size(); i++)
            if (p->idle[i].device == device) {
                l = p->idle[i];
                p->idle[i] = p->idle.back();
                p->idle.pop_back();
                return &l;
            }
    }
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, kCrcLaneHead + kCrcLaneData + 64, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        (void)hipHostFree(h);
        return nullptr;
    }
    l.host = (uint8_t *)h;
    l.dev = (uint8_t *)d;
    l.device = device;
    return &l;
}
// -> 0 and *out, or non-zero: the caller takes the general path
int crc32_lane(DeviceCtx *c, uint32_t value, const uint8_t *buf, size_t size, uint32_t *out) {
    const int mode = crc_lane_mode();
    if (mode == 0 || size > kCrcLaneData) return 1;
    CrcLane *l = crc_lane_for(ctx_device(c));
    if (!l) return 1;
    uint32_t *h_crc = (uint32_t *)l->host;
    uint64_t *h_off = (uint64_t *)(l->host + kCrcLaneSegs * 4);
    uint32_t *h_len = (uint32_t *)(l->host + kCrcLaneSegs * 12);
    const uint32_t nseg = (uint32_t)((size + kCrcLanePiece - 1) / kCrcLanePiece);
    for (uint32_t i = 0; i < nseg; i++) {
        h_off[i] = kCrcLaneHead + (uint64_t)i * kCrcLanePiece;
        const size_t left = size - (size_t)i * kCrcLanePiece;
        h_len[i] = (uint32_t)(left < kCrcLanePiece ? left : kCrcLanePiece);
    }
    memcpy(l->host + kCrcLaneHead, buf, size);
    hipStream_t s = MZ_HOST_STREAM;
    if (mode == 2) {
        if (mzhip_crc32_batch(l->dev, (const uint64_t *)(l->dev + kCrcLaneSegs * 4), (const uint32_t *)(l->dev + kCrcLaneSegs * 12), nseg, nullptr,
                              (uint32_t *)l->dev, s) != 0)
            return 2;
        if (hipStreamSynchronize(s) != hipSuccess) return 2;
    } else {
        Staging sc;
        if (sc.get(c, kCrcLaneHead + size) != 0) return 2;
        uint8_t *base = (uint8_t *)sc.p;
        if (hipMemcpyAsync(base + kCrcLaneSegs * 4, l->host + kCrcLaneSegs * 4, kCrcLaneHead - kCrcLaneSegs * 4 + size, hipMemcpyHostToDevice, s) != hipSuccess) return 2;
        if (mzhip_crc32_batch(base, (const uint64_t *)(base + kCrcLaneSegs * 4), (const uint32_t *)(base + kCrcLaneSegs * 12), nseg, nullptr, (uint32_t *)base, s) != 0)
            return 2;
        if (hipMemcpyAsync(h_crc, base, (size_t)nseg * 4, hipMemcpyDeviceToHost, s) != hipSuccess) return 2;
        if (hipStreamSynchronize(s) != hipSuccess) return 2;
    }
    uint32_t v = value;
    for (uint32_t i = 0; i < nseg; i++) v = crc32_combine(v, h_crc[i], h_len[i]);
    *out = v;
    return 0;
}
} // namespace

uint32_t mzhip_crc32_host(uint32_t value, const uint8_t *buf, size_t size) {
    if (size == 0) return value;
    if (size < MZHIP_CRC_HOST_BELOW) return crc32_fold_host(value, buf, size);
    DeviceCtx *c = nullptr;
    if (ctx_for_current(&c)) {
        crc_fault("no usable HIP device");
        return crc32_fold_host(value, buf, size);
    }
    if (size <= kCrcLaneData && crc_lane_mode() != 0) {
        if (crc_fault_injected()) {
            crc_fault("staging, copy or launch failed");
            return crc32_fold_host(value, buf, size);
        }
        uint32_t v = 0;
        const int lr = crc32_lane(c, value, buf, size, &v);
        if (lr == 0) return v;
        if (lr == 2) {
            (void)hipGetLastError();
            crc_fault("launch or wait failed");
            return crc32_fold_host(value, buf, size);
        }
        /* (no page-locked block to be had: the general path below) */
    }
    // segments of 256 KiB, one wave each; segment CRCs are chained with x^(8*len) shifts
    // (32-bit arithmetic on checksums only, no byte is touched on the host).
    const uint32_t seg = 256u << 10;
    const uint32_t nseg = (uint32_t)((size + seg - 1) / seg);
    const size_t meta = (size_t)nseg * (8 + 4 + 4);
    const size_t meta_pad = (meta + 63) & ~(size_t)63;
    Staging sc;
    uint64_t *h_off = (uint64_t *)malloc(meta_pad);
    bool ok = h_off != nullptr && sc.get(c, meta_pad + size) == 0 && !crc_fault_injected();
    uint32_t v = value;
    if (ok) {
        uint8_t *base = (uint8_t *)sc.p;
        uint32_t *h_len = (uint32_t *)(h_off + nseg);
        uint32_t *h_crc = h_len + nseg;
        for (uint32_t i = 0; i < nseg; i++) {
            h_off[i] = meta_pad + (uint64_t)i * seg;
            size_t left = size - (size_t)i * seg;
            h_len[i] = (uint32_t)(left < seg ? left : seg);
        }
        ok = mz_h2d(base, h_off, meta) == hipSuccess &&
             mz_h2d(base + meta_pad, buf, size) == hipSuccess;
        uint64_t *d_off = (uint64_t *)base;
        uint32_t *d_len = (uint32_t *)(d_off + nseg);
        uint32_t *d_crc = d_len + nseg;
        ok = ok && mzhip_crc32_batch(base, d_off, d_len, nseg, nullptr, d_crc, MZ_HOST_STREAM) == 0;
        ok = ok && mz_d2h(h_crc, d_crc, nseg * sizeof(uint32_t)) == hipSuccess;
        if (ok)
            for (uint32_t i = 0; i < nseg; i++) v = crc32_combine(v, h_crc[i], h_len[i]);
    }
    free(h_off);
    if (!ok) {
        crc_fault("staging, copy or launch failed");
        return crc32_fold_host(value, buf, size);
    }
    return v;
}

// a thread the shims start for a stream (shim_zlib.c: the window decoded ahead) works on the device of the thread that owns the stream
__attribute__((visibility("hidden"))) void mzhip_thread_use_device(int32_t dev) {
    if (dev >= 0) (void)hipSetDevice(dev);
}

// the failure a mz_crypt_crc32_update of this thread could not report (0 = none); reading clears it
__attribute__((visibility("hidden"))) int32_t mzhip_take_crc_fault(void) {
    const int32_t f = g_crc_fault;
    g_crc_fault = 0;
    return f;
}

} // extern "C"
