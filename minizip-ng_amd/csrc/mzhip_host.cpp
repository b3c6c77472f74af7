// mzhip_host.cpp -- host runtime of libmzhip.so that launches nothing itself: the per-thread error text, device queries, the
// per-thread stream pool, the checksums of a decoded window, the synchronous one-entry host-buffer calls that only call the
// batch launchers (what the vtbl shims call where the reference would call zlib / liblzma one entry at a time),
// and the RCCL gather.  Built by the host C++ compiler against <hip/hip_runtime_api.h>; mzhip_runtime.h declares what it
// shares with the kernels' translation unit (mzhip_kernels.hip + mzhip_launch.inc).
#include "mzhip_runtime.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>
#include <dlfcn.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace mzh;

__thread char mzh::g_err[256] = "";

int32_t mzh::fail(const char *what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -104; /* MZ_INTERNAL_ERROR */
}

extern "C" {

const char *mzhip_last_error(void) { return g_err; }
const char *mzhip_version(void) { return "mzhip 0.6 (gfx950)"; }

int32_t mzhip_device_count(void) {
    static std::atomic<int> known{0}; /* every open() of a codec stream asks: one runtime call per process is enough */
    if (known.load(std::memory_order_relaxed) > 0) return known.load(std::memory_order_relaxed);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipSuccess && n > 0) known.store(n);
    if (e != hipSuccess) {
        fail("hipGetDeviceCount", e);
        return -1;
    }
    return n;
}

/* The CPUs next to a device (the NUMA node its PCIe root hangs off), from sysfs: page-locked memory that the device
 * copies from and to, and the host threads that read it, belong there -- on a two-socket box the far socket costs a
 * third of the link rate and half of the readers' memcpy rate (profiles/r3/threads_numa.log). */
int32_t mzhip_device_local_cpus(int32_t device, char *cpulist, int32_t cap) {
    if (!cpulist || cap < 2) return -102;
    cpulist[0] = 0;
    char bdf[64] = "";
    HIP_TRY(hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), device));
    for (char *p = bdf; *p; p++)
        if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = fopen(path, "r");
    int node = -1;
    if (f) {
        if (fscanf(f, "%d", &node) != 1) node = -1;
        fclose(f);
    }
    if (node < 0) return 0; /* one node, or the platform does not say */
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bdf);
    f = fopen(path, "r");
    if (!f) return 0;
    if (!fgets(cpulist, cap, f)) cpulist[0] = 0;
    fclose(f);
    size_t n = strlen(cpulist);
    while (n && (cpulist[n - 1] == '\n' || cpulist[n - 1] == ' ')) cpulist[--n] = 0;
    return (int32_t)n;
}

int32_t mzhip_bind_thread_near_device(int32_t device, int32_t max_cpus) {
    char list[1024];
    const int32_t n = mzhip_device_local_cpus(device, list, (int32_t)sizeof(list));
    if (n <= 0) return n;
    cpu_set_t have, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(have), &have) != 0) return 0;
    int taken = 0;
    for (const char *p = list; *p;) { /* "64-127,192-255": the cores first, their second hardware threads behind them */
        char *e = nullptr;
        long a = strtol(p, &e, 10), b = a;
        if (e == p) break;
        if (*e == '-') b = strtol(e + 1, &e, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (CPU_ISSET((int)c, &have) && (max_cpus <= 0 || taken < max_cpus)) {
                CPU_SET((int)c, &want);
                taken++;
            }
        p = (*e == ',') ? e + 1 : e;
        if (*e != ',' ) break;
    }
    if (!taken) return 0; /* the thread may not run on any of them: left where it is */
    if (sched_setaffinity(0, sizeof(want), &want) != 0) return 0;
    return taken;
}

int32_t mzhip_init(int32_t device) {
    HIP_TRY(hipSetDevice(device));
    DeviceCtx *c = nullptr;
    return ctx_for_current(&c);
}

} // extern "C"

namespace {
// The synchronous host-buffer entry points (one entry at a time: what the vtbl shims call) run on the calling thread's
// own stream: copies and launches are ordered on it and only that stream is waited for, so two host
// threads never serialise on the null stream or on a device-wide synchronisation.
// (hipStreamPerThread itself was the first choice; with two host threads decoding entries at the same time it handed
// back garbage result words now and then -- tests/test_gpu_dropin.py::test_archives_through_unmodified_mz_zip, one run in
// three -- so the per-thread stream is one this library creates: a non-blocking stream per (host thread, device), made
// on first use.)
// A thread that exits hands its streams to a free list instead of leaking them (an application that makes a reader pool
// per archive used to leave one stream per exited thread behind); they are recycled, never destroyed: the
// scratch and work-queue caches remember stream identities ("the next launch is on the stream that used it last"), and a
// recycled stream keeps the order that reasoning relies on, where a destroyed one's handle could come back as a stranger.
struct StreamPool {
    std::mutex mu;
    std::vector<hipStream_t> idle[kMaxDevices];
};
static StreamPool *stream_pool() {
    static StreamPool *p = new StreamPool(); // (never deleted: thread_local destructors may run after static ones)
    return p;
}
struct ThreadStreams {
    hipStream_t s[kMaxDevices] = {};
    ~ThreadStreams() {
        StreamPool *p = stream_pool();
        std::lock_guard<std::mutex> g(p->mu);
        for (int d = 0; d < kMaxDevices; d++)
            if (s[d]) p->idle[d].push_back(s[d]);
    }
};
thread_local ThreadStreams t_streams;
} // namespace

hipStream_t mzh::mz_host_stream() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) return nullptr;
    if (!t_streams.s[d]) {
        StreamPool *p = stream_pool();
        {
            std::lock_guard<std::mutex> g(p->mu);
            if (!p->idle[d].empty()) {
                t_streams.s[d] = p->idle[d].back();
                p->idle[d].pop_back();
            }
        }
        if (!t_streams.s[d] && hipStreamCreateWithFlags(&t_streams.s[d], hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            t_streams.s[d] = nullptr; /* the null stream still works, only slower */
        }
    }
    return t_streams.s[d];
}
// CRC-32 of the new bytes of a window, [hist, out_len) of the device's copy at base + out_off, in the pieces the caller will
// hand to mz_crypt_crc32_update: the first seg_first bytes (what completes the piece the previous window left open), then
// seg_stride at a time, the rest; one launch.  sm = device room for seg_max offsets, lengths and results.
int32_t mzh::window_piece_crcs(uint8_t *base, size_t out_off, uint32_t hist, uint32_t out_len, uint32_t seg_first, uint32_t seg_stride,
                               uint32_t *seg_crc, uint32_t seg_cap, uint32_t *nseg, uint8_t *sm, size_t seg_max) {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint32_t pos = hist;
    const uint32_t first = seg_first < out_len - hist ? seg_first : out_len - hist;
    if (first) {
        off.push_back(out_off + pos);
        len.push_back(first);
        pos += first;
    }
    while (pos < out_len) {
        const uint32_t n = out_len - pos < seg_stride ? out_len - pos : seg_stride;
        off.push_back(out_off + pos);
        len.push_back(n);
        pos += n;
    }
    const uint32_t ns = (uint32_t)len.size();
    if (ns > seg_cap || ns > seg_max) return 0;
    uint64_t *d_off = (uint64_t *)sm;
    uint32_t *d_len = (uint32_t *)(sm + seg_max * 8), *d_crc = d_len + seg_max;
    HIP_TRY(mz_h2d(d_off, off.data(), (size_t)ns * 8));
    HIP_TRY(mz_h2d(d_len, len.data(), (size_t)ns * 4));
    const int32_t rc = mzhip_crc32_batch(base, d_off, d_len, ns, nullptr, d_crc, MZ_HOST_STREAM);
    if (rc) return rc;
    HIP_TRY(mz_d2h(seg_crc, d_crc, (size_t)ns * 4));
    if (nseg) *nseg = ns;
    return 0;
}

// CRC-32 and / or Adler-32 of the new bytes of a window, [hist, out_len) of the device's copy at base + out_off (the wrapper
// trailers of window mode: gzip's CRC-32, zlib's Adler-32 run over every window).  One buffer is one wave in K2 / K5, so
// the window is cut into 64 KiB pieces -- one launch each kind -- and the pieces' checksums are combined on the host
// (arithmetic on checksums only).  sm = device room for `room` offsets, lengths and results.
int32_t mzh::window_checksums(uint8_t *base, size_t out_off, uint32_t hist, uint32_t out_len, uint32_t *crc, uint32_t *adler, uint8_t *sm,
                              size_t room, hipStream_t st) {
    if (!st) st = MZ_HOST_STREAM;
    if (crc) *crc = 0u;
    if (adler) *adler = 1u;
    if ((!crc && !adler) || out_len <= hist) return 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    for (uint32_t pos = hist; pos < out_len;) {
        const uint32_t n = out_len - pos < 65536u ? out_len - pos : 65536u;
        off.push_back(out_off + pos);
        len.push_back(n);
        pos += n;
    }
    const uint32_t ns = (uint32_t)len.size();
    if (ns > room) return -104;
    uint64_t *d_off = (uint64_t *)sm;
    uint32_t *d_len = (uint32_t *)(sm + room * 8), *d_res = d_len + room;
    HIP_TRY(mz_h2d_on(st, d_off, off.data(), (size_t)ns * 8));
    HIP_TRY(mz_h2d_on(st, d_len, len.data(), (size_t)ns * 4));
    std::vector<uint32_t> h(ns);
    if (crc) {
        const int32_t rc = mzhip_crc32_batch(base, d_off, d_len, ns, nullptr, d_res, st);
        if (rc) return rc;
        HIP_TRY(mz_d2h_on(st, h.data(), d_res, (size_t)ns * 4));
        uint32_t v = h[0];
        for (uint32_t i = 1; i < ns; i++) v = crc32_combine(v, h[i], len[i]);
        *crc = v;
    }
    if (adler) {
        const int32_t rc = mzhip_adler32_batch(base, d_off, d_len, ns, d_res, st);
        if (rc) return rc;
        HIP_TRY(mz_d2h_on(st, h.data(), d_res, (size_t)ns * 4));
        uint32_t v = h[0];
        for (uint32_t i = 1; i < ns; i++) v = mzhip_adler32_combine(v, h[i], len[i]);
        *adler = v;
    }
    return 0;
}

extern "C" {

// One window of a stream that is decoded window by window (the READ shim's bounded-memory path): buf[0 .. state_in->out_pos)
// is the history the caller kept (the last 32 KiB it was given, nothing at the start of the stream), the new bytes land
// behind it, at most buf_cap bytes in all.  Returns the device verdict: MZHIP_OK (stream end), MZHIP_OUT_FULL (call again
// with state_out and the tail of buf as history), MZHIP_BUF_ERROR (call again with more input from state_out's block
// header on), or a data error.  *out_len = bytes valid in buf (history included), *crc = CRC-32 of the new bytes only.
static int32_t inflate_window_host(const uint8_t *in, uint32_t in_len, uint8_t *buf, uint32_t buf_cap,
                                       const mzhip_inflate_state *state_in, mzhip_inflate_state *state_out, uint32_t *out_len,
                                       uint32_t *in_used, uint32_t *crc, uint32_t *adler, uint32_t seg_first, uint32_t seg_stride,
                                       uint32_t *seg_crc, uint32_t seg_cap, uint32_t *nseg) {
    const uint32_t hist = state_in ? state_in->out_pos : 0u;
    struct Meta {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, in_used, crc;
        int32_t status;
        mzhip_inflate_state rs, st;
    };
    HostCall<Meta> hc;
    int32_t rc = ctx_for_current(&hc.c);
    if (rc) return rc;
    if (hist > buf_cap) return -102; /* MZ_PARAM_ERROR */
    // layout: [meta][in][buf][segment arrays][checksum arrays]
    const size_t seg_max = (seg_stride && seg_crc) ? (size_t)buf_cap / seg_stride + 3 : 0;
    const size_t ck_max = adler ? (size_t)buf_cap / 65536u + 3 : 0;
    Meta &m = hc.m;
    m.in_off = hc.take(in_len);
    m.out_off = hc.take((size_t)buf_cap + 16);
    const size_t o_seg = hc.take(seg_max * 16), o_ck = hc.take(ck_max * 16);
    m.in_len = in_len;
    m.out_cap = buf_cap;
    if (state_in) memcpy(&m.rs, state_in, sizeof(m.rs));
    give(nseg, 0u);
    give(adler, 1u);
    rc = hc.begin();
    if (rc) return rc;
    uint8_t *base = hc.at(0);
    Meta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (in_len) HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
    if (hist) HIP_TRY(mz_h2d(hc.at(m.out_off), buf, hist));
    rc = mzhip_inflate_resume_batch(base, &dm->in_off, &dm->in_len, base, &dm->out_off, &dm->out_cap, 1, &dm->out_len,
                                    &dm->in_used, &dm->crc, &dm->status, (const mzhip_inflate_state *)&dm->rs,
                                    /* no state asked for = the last call of a stream that ended short: the kernel then drops the
                                     * resumable rules (a stored block is taken as far as it goes) -- the pointer used to be
                                     * passed regardless, and a truncated stored stream in window mode lost its last bytes
                                     * (found by tests/test_gpu_dropin.py::test_truncation_accounting_window_mode, round 4) */
                                    state_out ? (mzhip_inflate_state *)&dm->st : nullptr, MZ_HOST_STREAM);
    if (rc) return rc;
    HIP_TRY(hc.fetch_meta());
    if (m.out_len > hist) HIP_TRY(mz_d2h(buf + hist, hc.at(m.out_off) + hist, m.out_len - hist));
    if (seg_max && m.out_len > hist) {
        rc = window_piece_crcs(base, m.out_off, hist, m.out_len, seg_first, seg_stride, seg_crc, seg_cap, nseg, hc.at(o_seg), seg_max);
        if (rc) return rc;
    }
    if (adler && m.out_len > hist) {
        rc = window_checksums(base, m.out_off, hist, m.out_len, nullptr, adler, hc.at(o_ck), ck_max);
        if (rc) return rc;
    }
    give(out_len, m.out_len);
    give(in_used, m.in_used);
    give(crc, m.crc);
    if (state_out) memcpy(state_out, &m.st, sizeof(m.st));
    return m.status;
}

} // extern "C"

// One whole entry from a host buffer through a batch launcher, as a batch of one: `launch` gets the staging buffer (what the
// meta block's offsets count from) and the meta block on the device.  max_out is the LZMA family's; an Adler-32 is asked for by
// inflate's zlib wrapper only.
struct WholeMeta {
    uint64_t in_off, out_off;
    int64_t max_out;
    uint32_t in_len, out_cap, out_len, in_used, crc;
    int32_t status;
    uint32_t adler, pad;
};
template <class Launch>
static int32_t decode_whole_host(Launch launch, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, int64_t max_out,
                                 uint32_t *out_len, uint32_t *in_used, uint32_t *crc, uint32_t *adler) {
    HostCall<WholeMeta> hc;
    WholeMeta &m = hc.m;
    m.in_off = hc.take(in_len);
    m.out_off = hc.take((size_t)out_cap + 16);
    m.max_out = max_out;
    m.in_len = in_len;
    m.out_cap = out_cap;
    int32_t rc = hc.begin();
    if (rc) return rc;
    uint8_t *base = hc.at(0);
    WholeMeta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (in_len) HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
    rc = launch(base, dm);
    if (rc) return rc;
    if (adler) { /* zlib wrapper: Adler-32 of the decoded bytes, reduced on the device as well */
        HIP_TRY(hipStreamSynchronize(MZ_HOST_STREAM));
        rc = mzhip_adler32_batch(base, &dm->out_off, &dm->out_len, 1, &dm->adler, MZ_HOST_STREAM);
        if (rc) return rc;
    }
    HIP_TRY(hc.wait_fetch_meta());
    if (m.out_len && out) HIP_TRY(mz_d2h(out, hc.at(m.out_off), m.out_len));
    give(out_len, m.out_len);
    give(in_used, m.in_used);
    give(crc, m.crc);
    give(adler, m.adler);
    return m.status;
}
// (inflate and bzip2 launchers take the same arguments)
#define MZ_LAUNCH_ONE(fn)                                                                                                       \
    [](uint8_t *base, WholeMeta *dm) {                                                                                          \
        return fn(base, &dm->in_off, &dm->in_len, base, &dm->out_off, &dm->out_cap, 1, &dm->out_len, &dm->in_used, &dm->crc, \
                  &dm->status, MZ_HOST_STREAM);                                                                                 \
    }
static int32_t lzma_family_host(int xz, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, int64_t max_out,
                                uint32_t *out_len, uint32_t *in_used, uint32_t *crc) {
    return decode_whole_host(
        [xz](uint8_t *base, WholeMeta *dm) {
            return (xz ? mzhip_xz_batch : mzhip_lzma_batch)(base, &dm->in_off, &dm->in_len, base, &dm->out_off, &dm->out_cap, &dm->max_out, 1,
                                                            &dm->out_len, &dm->in_used, &dm->crc, &dm->status, MZ_HOST_STREAM);
        },
        in, in_len, out, out_cap, max_out, out_len, in_used, crc, nullptr);
}

extern "C" {

/* include/mzhip.h: one entry point for a whole entry and for one window of it.  Fields behind `size` read as zero / NULL, so a
 * caller compiled against an older (shorter) struct keeps working when fields are appended. */
int32_t mzhip_inflate_host_a(const mzhip_inflate_host_args *ap) {
    if (!ap || ap->size < offsetof(mzhip_inflate_host_args, buf) + sizeof(void *) || ap->size > 4096u || (ap->size & 3u)) return -102; /* MZ_PARAM_ERROR */
    mzhip_inflate_host_args a;
    memset(&a, 0, sizeof(a));
    memcpy(&a, ap, ap->size < sizeof(a) ? ap->size : sizeof(a));
    if (!a.state_in && !a.state_out) {
        if (a.nseg) *a.nseg = 0; /* (no pieces of a whole entry: the READ shim asks the per-call CRCs of a window only) */
        return decode_whole_host(MZ_LAUNCH_ONE(mzhip_inflate_batch), a.in, a.in_len, a.buf, a.buf_cap, 0, a.out_len, a.in_used, a.crc, a.adler);
    }
    return inflate_window_host(a.in, a.in_len, a.buf, a.buf_cap, a.state_in, a.state_out, a.out_len, a.in_used, a.crc, a.adler,
                               a.seg_first, a.seg_stride, a.seg_crc, a.seg_cap, a.nseg);
}

int32_t mzhip_lzma_host(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, int64_t max_out,
                        uint32_t *out_len, uint32_t *in_used, uint32_t *crc) {
    return lzma_family_host(0, in, in_len, out, out_cap, max_out, out_len, in_used, crc);
}

int32_t mzhip_xz_host(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, int64_t max_out,
                      uint32_t *out_len, uint32_t *in_used, uint32_t *crc) {
    return lzma_family_host(1, in, in_len, out, out_cap, max_out, out_len, in_used, crc);
}

// One bzip2 stream (ZIP method 12) from a host buffer.
int32_t mzhip_bzip2_host(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len, uint32_t *in_used,
                         uint32_t *crc) {
    return decode_whole_host(MZ_LAUNCH_ONE(mzhip_bzip2_batch), in, in_len, out, out_cap, 0, out_len, in_used, crc, nullptr);
}

int32_t mzhip_zstd_host(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len, uint32_t *in_used,
                        uint32_t *crc) {
    return decode_whole_host(MZ_LAUNCH_ONE(mzhip_zstd_batch), in, in_len, out, out_cap, 0, out_len, in_used, crc, nullptr);
}

// One ZIP method-14 payload from a host buffer.
int32_t mzhip_lzma_encode_host(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len,
                               uint32_t *crc) {
    return mzhip_lzma_encode_host_preset(in, in_len, 1, out, out_cap, out_len, crc);
}

int32_t mzhip_lzma_encode_host_preset(const uint8_t *in, uint32_t in_len, int32_t preset, uint8_t *out, uint32_t out_cap,
                                      uint32_t *out_len, uint32_t *crc) {
    struct Meta {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, crc;
        int32_t status;
    };
    HostCall<Meta> hc;
    Meta &m = hc.m;
    m.in_len = in_len;
    m.out_cap = in_len + in_len / 8 + 1024;
    m.in_off = hc.take(in_len, 64);
    m.out_off = hc.take(m.out_cap, 64);
    int32_t rc = hc.begin();
    if (rc) return rc;
    uint8_t *base = hc.at(0);
    Meta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (in_len) HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
    rc = mzhip_lzma_encode_batch_preset(base, &dm->in_off, &dm->in_len, in_len, base, &dm->out_off, &dm->out_cap, nullptr, 1,
                                        preset, &dm->out_len, &dm->crc, &dm->status, MZ_HOST_STREAM);
    if (rc) return rc;
    HIP_TRY(hc.wait_fetch_meta());
    if (m.status == 0 && m.out_len > out_cap) m.status = MZHIP_STATUS_OUT_FULL;
    if (m.status == 0 && m.out_len) HIP_TRY(mz_d2h(out, hc.at(m.out_off), m.out_len));
    give(out_len, m.out_len);
    give(crc, m.crc);
    return m.status;
}

// One ZIP method-12 payload (a bzip2 stream) from a host buffer.
int32_t mzhip_bzip2_encode_host(const uint8_t *in, uint32_t in_len, int32_t level, uint8_t *out, uint32_t out_cap, uint32_t *out_len,
                                uint32_t *crc) {
    struct Meta {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, crc;
        int32_t status;
    };
    const uint64_t bound = mzhip_bzip2_encode_bound(in_len, level);
    if (bound == 0 || bound > 0xFFFFFFFFull) return -102; /* MZ_PARAM_ERROR: no such level (or an entry whose bound needs 33 bits) */
    HostCall<Meta> hc;
    Meta &m = hc.m;
    m.in_len = in_len;
    m.out_cap = (uint32_t)bound;
    m.in_off = hc.take(in_len, 64);
    m.out_off = hc.take(m.out_cap, 64);
    int32_t rc = hc.begin();
    if (rc) return rc;
    uint8_t *base = hc.at(0);
    Meta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (in_len) HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
    rc = mzhip_bzip2_encode_batch(base, &dm->in_off, &dm->in_len, in_len, base, &dm->out_off, &dm->out_cap, 1, level, &dm->out_len,
                                  &dm->crc, &dm->status, MZ_HOST_STREAM);
    if (rc) return rc;
    HIP_TRY(hc.wait_fetch_meta());
    if (m.status == 0 && m.out_len > out_cap) {
        m.status = MZHIP_STATUS_OUT_FULL;
        m.out_len = 0;
    }
    if (m.status == 0 && m.out_len) HIP_TRY(mz_d2h(out, hc.at(m.out_off), m.out_len));
    give(out_len, m.out_len);
    give(crc, m.crc);
    return m.status;
}

// One ZIP method-93 payload (a Zstandard frame) from a host buffer.
int32_t mzhip_zstd_encode_host(const uint8_t *in, uint32_t in_len, int32_t level, uint32_t flags, uint8_t *out, uint32_t out_cap,
                               uint32_t *out_len, uint32_t *crc) {
    struct Meta {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, crc;
        int32_t status;
    };
    const uint64_t bound = mzhip_zstd_encode_bound(in_len);
    if (level < -1 || level > 22 || bound > 0xFFFFFFFFull) return -102; /* MZ_PARAM_ERROR: no such level (or an entry whose bound needs 33 bits) */
    HostCall<Meta> hc;
    Meta &m = hc.m;
    m.in_len = in_len;
    m.out_cap = (uint32_t)bound;
    m.in_off = hc.take(in_len, 64);
    m.out_off = hc.take(m.out_cap, 64);
    int32_t rc = hc.begin();
    if (rc) return rc;
    uint8_t *base = hc.at(0);
    Meta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (in_len) HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
    rc = mzhip_zstd_encode_batch(base, &dm->in_off, &dm->in_len, in_len, base, &dm->out_off, &dm->out_cap, 1, level, flags, &dm->out_len,
                                 &dm->crc, &dm->status, MZ_HOST_STREAM);
    if (rc) return rc;
    HIP_TRY(hc.wait_fetch_meta());
    if (m.status == 0 && m.out_len > out_cap) {
        m.status = MZHIP_STATUS_OUT_FULL;
        m.out_len = 0;
    }
    if (m.status == 0 && m.out_len) HIP_TRY(mz_d2h(out, hc.at(m.out_off), m.out_len));
    give(out_len, m.out_len);
    give(crc, m.crc);
    return m.status;
}

// ... then the index over all blocks and the stream footer (host arithmetic only: a few dozen bytes)
int32_t mzhip_xz_encode_finish_host(const uint64_t *unpadded_size, const uint64_t *uncompressed_size, uint32_t nblocks, uint8_t *out,
                                    uint32_t out_cap, uint32_t *out_len) {
    std::vector<uint8_t> idx;
    auto vli = [&](uint64_t v) {
        while (v >= 0x80) { idx.push_back((uint8_t)(v | 0x80)); v >>= 7; }
        idx.push_back((uint8_t)v);
    };
    idx.push_back(0x00);
    vli(nblocks);
    for (uint32_t i = 0; i < nblocks; i++) {
        vli(unpadded_size[i]);
        vli(uncompressed_size[i]);
    }
    while (idx.size() & 3u) idx.push_back(0);
    uint8_t c4[4];
    put_le32(c4, mzhip_crc32_host(0, idx.data(), idx.size()));
    idx.insert(idx.end(), c4, c4 + 4);
    uint8_t ft[12];
    put_le32(ft + 4, (uint32_t)(idx.size() / 4 - 1));
    ft[8] = 0x00;
    ft[9] = 0x01;
    put_le32(ft, mzhip_crc32_host(0, ft + 4, 6));
    ft[10] = 'Y';
    ft[11] = 'Z';
    if (idx.size() + 12 > out_cap) return MZHIP_STATUS_OUT_FULL;
    memcpy(out, idx.data(), idx.size());
    memcpy(out + idx.size(), ft, 12);
    if (out_len) *out_len = (uint32_t)idx.size() + 12;
    return 0;
}

/* The per-archive result gather behind the C ABI (north_star: "RCCL over xGMI only for the final per-archive CRC
 * gather").  libmzhip.so does not link RCCL: the library is opened with dlopen() when the first call with a communicator needs
 * it, so a single-GPU application never loads it. */
namespace {
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
nccl_allgather_fn g_nccl_allgather = nullptr;
std::once_flag g_nccl_once;
void nccl_load() {
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            g_nccl_allgather = (nccl_allgather_fn)dlsym(h, "ncclAllGather");
            if (g_nccl_allgather) return;
        }
    }
}
} // namespace

int32_t mzhip_gather_results(void *comm, int32_t rank, int32_t world, const int64_t *bounds, const uint32_t *d_crc, const int32_t *d_status,
                             uint32_t *d_crc_all, int32_t *d_status_all, void *stream) {
    if (world < 1 || rank < 0 || rank >= world || !bounds || !d_crc_all || !d_status_all) return -102; /* MZ_PARAM_ERROR */
    hipStream_t s = (hipStream_t)stream;
    /* every rank's slice, not only this one's: a table that runs backwards anywhere would turn into a huge copy count below */
    if (bounds[0] < 0) return -102;
    for (int32_t r = 0; r < world; r++)
        if (bounds[r + 1] < bounds[r] || bounds[r + 1] - bounds[r] > (int64_t)0x3FFFFFFF) return -102;
    const int64_t n_local = bounds[rank + 1] - bounds[rank];
    if (n_local > 0 && (!d_crc || !d_status)) return -102;
    if (world == 1 || !comm) {
        if (world != 1) return -102; /* several ranks need the job's communicator */
        if (n_local) {
            HIP_TRY(hipMemcpyAsync(d_crc_all + bounds[0], d_crc, (size_t)n_local * 4, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_status_all + bounds[0], d_status, (size_t)n_local * 4, hipMemcpyDeviceToDevice, s));
        }
        return 0;
    }
    std::call_once(g_nccl_once, nccl_load);
    if (!g_nccl_allgather) {
        snprintf(g_err, sizeof(g_err), "mzhip_gather_results: librccl.so could not be loaded (dlopen)");
        return -109; /* MZ_SUPPORT_ERROR */
    }
    int64_t mx = 0;
    for (int32_t r = 0; r < world; r++) mx = std::max(mx, bounds[r + 1] - bounds[r]);
    if (mx == 0) return 0;
    /* ncclAllGather moves equal blocks: every rank sends {crc[0 .. mx), status[0 .. mx)} (its slice, padded), one collective; the
     * slices are then copied to where the table wants them.  The block buffers come from the scratch cache of the device. */
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    ScratchLease sc;
    rc = sc.get(ctx_scratch(c), (size_t)(world + 1) * 2 * (size_t)mx * 4, s);
    if (rc) return rc;
    uint32_t *send = (uint32_t *)sc.p, *recv = send + 2 * mx;
    hipError_t e = hipSuccess;
    if (n_local) {
        e = hipMemcpyAsync(send, d_crc, (size_t)n_local * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(send + mx, d_status, (size_t)n_local * 4, hipMemcpyDeviceToDevice, s);
    }
    int nr = 0;
    if (e == hipSuccess) nr = g_nccl_allgather(send, recv, (size_t)(2 * mx), 2 /* ncclInt32 */, comm, s);
    for (int32_t r = 0; e == hipSuccess && nr == 0 && r < world; r++) {
        const int64_t cnt = bounds[r + 1] - bounds[r];
        if (!cnt) continue;
        e = hipMemcpyAsync(d_crc_all + bounds[r], recv + (size_t)r * 2 * mx, (size_t)cnt * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_status_all + bounds[r], recv + (size_t)r * 2 * mx + mx, (size_t)cnt * 4, hipMemcpyDeviceToDevice, s);
    }
    if (e != hipSuccess) return fail("mzhip_gather_results", e);
    if (nr != 0) {
        snprintf(g_err, sizeof(g_err), "mzhip_gather_results: ncclAllGather returned %d", nr);
        return -104; /* MZ_INTERNAL_ERROR */
    }
    return 0;
}

} // extern "C"
