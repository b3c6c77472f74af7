// mzhip_launch.inc -- the launch side of libmzhip.so's runtime, textually included by mzhip_kernels.hip: everything whose body
// names a kernel, a kernel argument struct or a constant of a *_core.h.  Device context, the launchers of the batch C ABI
// (include/mzhip.h), and the host-buffer entry points that launch kernels themselves (the many-wave inflate, the resumable
// LZMA coders, the .xz writer, the DEFLATE segment writer); the scratch and work-queue caches every launch leases from are
// mzhip_slots.inc, defined here.  It holds no device code.  The rest of the runtime -- stream pool, staging, CRC lane, gather,
// prime caches -- is built apart from the kernels (mzhip_host.cpp, mzhip_crc_host.cpp, mzhip_prime.cpp); mzhip_runtime.h
// declares what crosses.
// ---------------------------------------------------------------------------------- host

#define MZHIP_SLOTS_DEFINE
#include "mzhip_slots.inc"

using namespace mzh;

namespace mzh {

struct DeviceCtx {
    bool ready = false;
    mzhip_crc_tables *d_tabs = nullptr;
    uint64_t *d_tab64 = nullptr;
    ScratchCache scratch;  // per-launch scratch (K1 records, K4 / K6 tokens, ...) and the host-buffer calls' staging
    CounterCache counters; // the work-queue heads of the launches
    int cu_count = 0;
    int inflate_wgs_per_cu = 1;
    // the four-candidate classes of K4 / the LZ tokenizer need > 64 KiB of dynamic LDS per workgroup: asked for once per
    // device; 0 = not asked yet, 1 = granted, -1 = refused (the one-candidate class is used instead)
    std::atomic<int> big_lds_deflate{0}, big_lds_deflate_cost{0}, big_lds_tok{0};
};
} // namespace mzh

namespace {

// may this device run `kernel` with `bytes` of dynamic LDS per workgroup?  (asked once per device and kernel)
bool big_lds_ok(std::atomic<int> &state, const void *kernel, size_t bytes) {
    int st = state.load(std::memory_order_acquire);
    if (st == 0) {
        const bool ok = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
        if (!ok) (void)hipGetLastError(); /* (a launch that is refused all the same turns the state to -1, too) */
        st = ok ? 1 : -1;
        state.store(st, std::memory_order_release);
    }
    return st > 0;
}

DeviceCtx g_ctx[kMaxDevices];

} // namespace

int mzh::ctx_device(const DeviceCtx *c) { return (int)(c - g_ctx); }
ScratchCache *mzh::ctx_scratch(DeviceCtx *c) { return &c->scratch; }

int32_t mzh::ctx_for_current(DeviceCtx **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) {
        snprintf(g_err, sizeof(g_err), "device index %d out of range", dev);
        return -102;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceCtx &c = g_ctx[dev];
    if (!c.ready) {
        mzhip_crc_tables h;
        mzhip_crc_tables_init(&h);
        HIP_TRY(hipMalloc((void **)&c.d_tabs, sizeof(h)));
        HIP_TRY(hipMemcpy(c.d_tabs, &h, sizeof(h), hipMemcpyHostToDevice));
        uint64_t t64[256];
        mzhip_crc64_table_init(t64);
        HIP_TRY(hipMalloc((void **)&c.d_tab64, sizeof(t64)));
        HIP_TRY(hipMemcpy(c.d_tab64, t64, sizeof(t64), hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc((void **)&c.counters.words, 2 * MZ_NUM_COUNTERS * sizeof(uint32_t)));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        c.cu_count = prop.multiProcessorCount;
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inflate_batch<true>, MZ_WAVES_PER_WG * 64,
                                                         MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * MZ_LDS_STRIDE) == hipSuccess &&
            nb > 0)
            c.inflate_wgs_per_cu = nb;
        c.ready = true;
    }
    *out = &c;
    return 0;
}

namespace {

// The prologue of a launcher: the current device's context, the caller's stream and, where the kernel has a work queue, its
// zeroed heads -- given back (an event recorded behind the launch) when the launcher returns.
struct Launch {
    DeviceCtx *c = nullptr;
    hipStream_t s = nullptr;
    CounterLease head;
    int32_t begin(void *stream, bool work_queue = true) {
        const int32_t rc = ctx_for_current(&c);
        if (rc) return rc;
        s = (hipStream_t)stream;
        return work_queue ? head.get(&c->counters, s) : 0;
    }
};

// The epilogue of a launcher that leased scratch: the lease is given back (its event recorded behind the launch) whatever
// came of the launch; a launch error wins over a release error, which wins over success.
int32_t launched(const char *what, hipError_t le, ScratchLease &sc) {
    const int32_t rr = sc.release();
    return le != hipSuccess ? fail(what, le) : rr;
}

// Persistent waves: the workgroups the work needs, at most the ones that are resident at once (fill the chip once).
uint32_t resident_grid(uint64_t need, uint64_t resident) { return (uint32_t)(need < resident ? need : resident); }

// The entry table of a batch call (EntryTable, mzhip_kernels.hip) from the call's arguments; a call whose ABI lacks one of
// the arrays passes nullptr for it, in so many words.  `counter` is the launcher's to set.
void set_fields(EntryTable &a, const DeviceCtx *c, const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, uint32_t *d_out_len, uint32_t *d_in_used,
                uint32_t *d_crc, int32_t *d_status) {
    a.in = (const uint8_t *)d_in;
    a.in_off = d_in_off;
    a.in_len = d_in_len;
    a.out = (uint8_t *)d_out;
    a.out_off = d_out_off;
    a.out_cap = d_out_cap;
    a.n = n;
    a.out_len = d_out_len;
    a.in_used = d_in_used;
    a.crc = d_crc;
    a.status = d_status;
    a.tabs = c->d_tabs;
}

template <class A>
struct Kernel {
    void (*fn)(A);
    const char *name;
};
#define MZ_KERNEL(k) {k, #k}

uint32_t grid_for(const DeviceCtx *c, uint32_t n) {
    const uint32_t wgs_needed = (n + MZ_WAVES_PER_WG - 1) / MZ_WAVES_PER_WG;
    /* (Round 4 measured "balanced rounds" -- just enough waves to fill ceil(n / resident) rounds evenly, 3128 instead of
     * 4096 for one rank's 12 500 entries at N = 8: 245 GiB/s against 279.  A nearly empty last round on a full chip beats
     * full rounds on three quarters of it: profiles/r4/ab_balanced_rounds.log.) */
    return resident_grid(wgs_needed ? wgs_needed : 1u, (uint32_t)(c->cu_count * c->inflate_wgs_per_cu));
}

// ZipCrypto, both directions: a lane per entry; d_header is the write side's (null on the way in)
int32_t pkcrypt_batch(void (*kernel)(PkcryptArgs), const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                      const uint64_t *d_out_off, uint32_t n, const uint8_t *password, uint32_t password_len,
                      const uint32_t *d_verify, const uint8_t *d_header, uint32_t *d_out_len, int32_t *d_status, void *stream) {
    if (!password) return MZ_CRYPT_PARAM_ERROR;
    if (n == 0) return 0;
    Launch L;
    const int32_t rc = L.begin(stream, false);
    if (rc) return rc;
    PkcryptArgs a{};
    set_fields(a, L.c, d_in, d_in_off, d_in_len, d_out, d_out_off, nullptr, n, d_out_len, nullptr, nullptr, d_status);
    uint32_t keys[3];
    mz_pk_init_keys_host(password, password_len, keys);
    a.k0 = keys[0];
    a.k1 = keys[1];
    a.k2 = keys[2];
    a.verify = d_verify;
    a.header = d_header;
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, L.s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// WinZip-AES, both directions: the entries' keys (four lanes an entry), CTR over the payloads (the work queue), the HMAC
// a lane per entry -- on the way in behind the CTR kernel: it authenticates the ciphertext that kernel wrote; d_salt is the
// write side's (null on the way in)
int32_t wzaes_batch(const Kernel<WzaesArgs> (&k)[3], const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                    const uint8_t *d_strength, const uint8_t *d_salt, void *d_out, const uint64_t *d_out_off, uint32_t n,
                    const uint8_t *password, uint32_t password_len, uint32_t *d_out_len, int32_t *d_status, void *stream) {
    if (!password || password_len > MZ_WZAES_PW_MAX) return MZ_CRYPT_PARAM_ERROR;
    if (n == 0) return 0;
    if (n > 0x3FFFFFFFu) return MZ_CRYPT_PARAM_ERROR; /* four lane slots per entry in a 32-bit thread index */
    Launch L;
    int32_t rc = L.begin(stream);
    if (rc) return rc;
    WzaesArgs a{}; /* (the password's unused bytes are zero with it) */
    set_fields(a, L.c, d_in, d_in_off, d_in_len, d_out, d_out_off, nullptr, n, d_out_len, nullptr, nullptr, d_status);
    a.strength = d_strength;
    a.salt = d_salt;
    a.password_len = password_len;
    memcpy(a.password, password, password_len);
    a.counter = L.head.p;
    ScratchLease sc;
    rc = sc.get(&L.c->scratch, (size_t)n * sizeof(mz_wzaes_entry_keys), L.s);
    if (rc) return rc;
    a.keys = (mz_wzaes_entry_keys *)sc.p;
    int at = 0;
    hipLaunchKernelGGL(k[0].fn, dim3((uint32_t)(((uint64_t)n * 4u + 255u) / 256u)), dim3(256), 0, L.s, a);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) {
        at = 1;
        hipLaunchKernelGGL(k[1].fn, dim3(grid_for(L.c, n)), dim3(MZ_WAVES_PER_WG * 64), 0, L.s, a);
        le = hipGetLastError();
    }
    if (le == hipSuccess) {
        at = 2;
        hipLaunchKernelGGL(k[2].fn, dim3((n + 255) / 256), dim3(256), 0, L.s, a);
        le = hipGetLastError();
    }
    return launched(k[at].name, le, sc);
}

// "A wave per entry, single-wave workgroups, `per_cu` of them per CU, `stride` bytes of HBM scratch per resident wave":
// bzip2 and Zstandard decode, bzip2 encode.  grid = min(n, resident), so a small batch costs a small scratch.
uint32_t wave_grid(const DeviceCtx *c, uint32_t n, uint32_t per_cu) { return resident_grid(n, (uint32_t)c->cu_count * per_cu); }

// behind the ..._launch_geometry calls: that grid on the current device, 0 without one or for arguments the launcher refuses
uint32_t geometry_grid(bool args_ok, uint32_t n, uint32_t per_cu, uint32_t *grid) {
    DeviceCtx *c = nullptr;
    const uint32_t g = (args_ok && ctx_for_current(&c) == 0) ? wave_grid(c, n, per_cu) : 0u;
    if (grid) *grid = g;
    return g;
}

// the launcher: `a` arrives value-initialised with the kernel's own fields set; table, head, scratch slice and launch are here
template <class A>
int32_t wave_per_entry_batch(const Kernel<A> &k, A &a, uint32_t per_cu, size_t stride, const void *d_in, const uint64_t *d_in_off,
                             const uint32_t *d_in_len, void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n,
                             uint32_t *d_out_len, uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    if (n == 0) return 0;
    Launch L;
    int32_t rc = L.begin(stream);
    if (rc) return rc;
    set_fields(a, L.c, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, d_in_used, d_crc, d_status);
    a.counter = L.head.p;
    const uint32_t grid = wave_grid(L.c, n, per_cu);
    ScratchLease sc;
    rc = sc.get(&L.c->scratch, (size_t)grid * stride, L.s);
    if (rc) return rc;
    a.scratch = (uint8_t *)sc.p;
    hipLaunchKernelGGL(k.fn, dim3(grid), dim3(64), 0, L.s, a);
    return launched(k.name, hipGetLastError(), sc);
}

} // namespace

extern "C" {

void mzhip_inflate_launch_geometry(uint32_t n, uint32_t *grid, uint32_t *waves_per_wg, uint32_t *lds_bytes) {
    DeviceCtx *c = nullptr;
    uint32_t g = 0;
    if (ctx_for_current(&c) == 0) g = grid_for(c, n);
    if (grid) *grid = g;
    if (waves_per_wg) *waves_per_wg = MZ_WAVES_PER_WG;
    if (lds_bytes) *lds_bytes = (uint32_t)(MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * MZ_LDS_STRIDE);
}

int32_t mzhip_inflate_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                            const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, uint32_t *d_out_len,
                            uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    return mzhip_inflate_resume_batch(d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, d_in_used, d_crc,
                                      d_status, nullptr, nullptr, stream);
}

int32_t mzhip_inflate_resume_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                                   const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, uint32_t *d_out_len,
                                   uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, const mzhip_inflate_state *d_resume,
                                   mzhip_inflate_state *d_stop, void *stream) {
    static_assert(sizeof(mzhip_inflate_state) == sizeof(mz_inflate_state), "mzhip.h and inflate_core.h describe the same four words");
    if (n == 0) return 0;
    Launch L;
    int32_t rc = L.begin(stream);
    if (rc) return rc;
    InflateArgs a{};
    set_fields(a, L.c, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, d_in_used, d_crc, d_status);
    a.counter = L.head.p;
    a.resume = (const mz_inflate_state *)d_resume;
    a.stop = (mz_inflate_state *)d_stop;
    const size_t lds = MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * MZ_LDS_STRIDE;
    const uint32_t grid = grid_for(L.c, n);
    ScratchLease sc; /* the step records of the chase window: MZ_REC_BYTES per wave of the launch (176 KiB x 4096 resident waves at most) */
    rc = sc.get(&L.c->scratch, (size_t)grid * MZ_WAVES_PER_WG * MZ_REC_BYTES + 1024, L.s);
    if (rc) return rc;
    a.rec = (uint8_t *)sc.p;
    if (a.resume || a.stop) hipLaunchKernelGGL(k_inflate_batch<true>, dim3(grid), dim3(MZ_WAVES_PER_WG * 64), lds, L.s, a);
    else hipLaunchKernelGGL(k_inflate_batch<false>, dim3(grid), dim3(MZ_WAVES_PER_WG * 64), lds, L.s, a);
    return launched("k_inflate_batch", hipGetLastError(), sc);
}

// CRC-32 (d_init: the values to go on from, or null) and Adler-32 of n byte ranges, a wave each
static int32_t checksum_batch(void (*kernel)(CrcArgs), const void *d_buf, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                              const uint32_t *d_init, uint32_t *d_sum, void *stream) {
    if (n == 0) return 0;
    Launch L;
    const int32_t rc = L.begin(stream);
    if (rc) return rc;
    CrcArgs a{};
    a.buf = (const uint8_t *)d_buf;
    a.off = d_off;
    a.len = d_len;
    a.n = n;
    a.init = d_init;
    a.crc = d_sum;
    a.counter = L.head.p;
    a.tabs = L.c->d_tabs;
    hipLaunchKernelGGL(kernel, dim3(grid_for(L.c, n)), dim3(MZ_WAVES_PER_WG * 64), 0, L.s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int32_t mzhip_crc32_batch(const void *d_buf, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                          const uint32_t *d_init, uint32_t *d_crc, void *stream) {
    return checksum_batch(k_crc32_batch, d_buf, d_off, d_len, n, d_init, d_crc, stream);
}

int32_t mzhip_adler32_batch(const void *d_buf, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                            uint32_t *d_adler, void *stream) {
    return checksum_batch(k_adler32_batch, d_buf, d_off, d_len, n, nullptr, d_adler, stream);
}

static int32_t lzma_family_batch(int xz, const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                                 const uint64_t *d_out_off, const uint32_t *d_out_cap, const int64_t *d_max_out, uint32_t n,
                                 uint32_t *d_out_len, uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    if (n == 0) return 0;
    Launch L;
    int32_t rc = L.begin(stream);
    if (rc) return rc;
    DeviceCtx *c = L.c;
    hipStream_t s = L.s;
    LzmaArgs a{}; /* sprobs, retry_list, retry_n stay null unless the slot kernel runs */
    set_fields(a, c, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, d_in_used, d_crc, d_status);
    a.max_out = d_max_out;
    a.counter = L.head.p;
    a.tab64 = c->d_tab64;
    /* 16 KiB LDS per wave -> 10 single-wave workgroups per CU (K3); 17.6 KiB -> 8 (.xz) */
    uint32_t resident = (uint32_t)c->cu_count * (xz ? 8u : 10u);
#ifdef MZ_LZMA_RESIDENT /* measurement builds: single-wave workgroups per CU that really fit (LDS and registers) */
    if (!xz) resident = (uint32_t)c->cu_count * MZ_LZMA_RESIDENT;
#endif
    const uint32_t grid = resident_grid(n, resident);
    ScratchLease sc; /* 12 KiB per resident wave: the literal model's upper half for streams with lc + lp = 4 */
#if defined(MZ_LZMA_NO_SLOT_KERNEL)
    const bool two_step = false;
#else
    const bool two_step = !xz;
#endif
    if (two_step) {
        /* K3: the slot kernel over every entry (16 waves per CU), then the full-model kernel over the entries it gave back */
#ifndef MZ_LZMA_SLOT_WGS
#define MZ_LZMA_SLOT_WGS 4u /* workgroups of four waves per CU (measurement builds: 1 or 2 -- how fast is a stream's chain of decisions
                               when fewer waves share the SIMD's issue port?  profiles/r6/README.md, K3) */
#endif
        const uint32_t grid_s = resident_grid((n + 3u) / 4u, (uint32_t)c->cu_count * MZ_LZMA_SLOT_WGS); /* workgroups of four waves */
        const size_t sp_bytes = (size_t)grid_s * 4u * MZ_LZMA_SPROBS * sizeof(uint16_t);
        const size_t xp_bytes = (size_t)grid * MZ_LZMA_XPROBS * sizeof(uint16_t);
        rc = sc.get(&c->scratch, sp_bytes + xp_bytes + (size_t)n * 4 + 256, s);
        if (rc) return rc;
        uint8_t *scratch = (uint8_t *)sc.p;
        a.sprobs = (uint16_t *)scratch;
        a.xprobs = (uint16_t *)(scratch + sp_bytes);
        uint32_t *list = (uint32_t *)(scratch + sp_bytes + xp_bytes);
        a.retry_list = list + 64;
        a.retry_n = list; /* one word, zeroed with the launch */
        hipError_t he = hipMemsetAsync(list, 0, 256, s);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(k_lzma_slot_batch, dim3(grid_s), dim3(256), 0, s, a);
            he = hipGetLastError();
        }
        if (he == hipSuccess) {
            a.counter = L.head.p + 1; /* the second head of the lease */
            hipLaunchKernelGGL(k_lzma_batch, dim3(grid), dim3(64), 0, s, a);
            he = hipGetLastError();
        }
        return launched("k_lzma_slot_batch", he, sc);
    }
    rc = sc.get(&c->scratch, (size_t)grid * MZ_LZMA_XPROBS * sizeof(uint16_t), s);
    if (rc) return rc;
    a.xprobs = (uint16_t *)sc.p;
    if (xz)
        hipLaunchKernelGGL(k_xz_batch, dim3(grid), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL(k_lzma_batch, dim3(grid), dim3(64), 0, s, a);
    return launched("k_lzma_batch", hipGetLastError(), sc);
}

int32_t mzhip_lzma_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                         const uint64_t *d_out_off, const uint32_t *d_out_cap, const int64_t *d_max_out, uint32_t n,
                         uint32_t *d_out_len, uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    return lzma_family_batch(0, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_max_out, n, d_out_len, d_in_used,
                             d_crc, d_status, stream);
}

int32_t mzhip_xz_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                       const uint64_t *d_out_off, const uint32_t *d_out_cap, const int64_t *d_max_out, uint32_t n,
                       uint32_t *d_out_len, uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    return lzma_family_batch(1, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_max_out, n, d_out_len, d_in_used,
                             d_crc, d_status, stream);
}

/* bzip2: the inverse BWT of a block needs MZ_BZ_SCRATCH_BYTES = 4 518 144 bytes of HBM per resident wave (4 bytes of link
 * and first-column byte per symbol of a 900 000-symbol block, the block's 900 000 bytes, 18 002 selectors).  8 single-wave
 * workgroups per CU, two per SIMD: the chain walk is one dependent load per byte, so a wave mostly waits and more waves
 * would hide more of it -- LDS (10.4 KiB per wave) would allow 15 -- but every further wave per CU costs 1.1 GiB of
 * scratch on a 256-CU device; 8 per CU is 8.6 GiB for a full grid.  grid = min(n, resident): a small batch costs a small
 * scratch. */
#define MZ_BZ_WAVES_PER_CU 8u

void mzhip_bzip2_launch_geometry(uint32_t n, uint32_t *grid, uint64_t *scratch_bytes) {
    const uint32_t g = geometry_grid(true, n, MZ_BZ_WAVES_PER_CU, grid);
    if (scratch_bytes) *scratch_bytes = (uint64_t)g * MZ_BZ_SCRATCH_BYTES;
}

int32_t mzhip_bzip2_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                          const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, uint32_t *d_out_len,
                          uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    static const Kernel<WaveScratchArgs> k = MZ_KERNEL(k_bzip2_batch);
    WaveScratchArgs a{};
    return wave_per_entry_batch(k, a, MZ_BZ_WAVES_PER_CU, MZ_BZ_SCRATCH_BYTES, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n,
                                d_out_len, d_in_used, d_crc, d_status, stream);
}

/* zstd: the literals of a block (at most 128 KiB) are decoded into HBM, MZ_ZS_SCRATCH_BYTES = 131 328 per resident wave.
 * 8 single-wave workgroups per CU, two per SIMD, as for bzip2: the sequence machine is a chain of dependent LDS reads, so a
 * wave mostly waits; LDS (11.1 KiB per wave) would allow 14.  A full grid on a 256-CU device holds 256 MiB of scratch.
 * grid = min(n, resident). */
#define MZ_ZS_WAVES_PER_CU 8u

void mzhip_zstd_launch_geometry(uint32_t n, uint32_t *grid, uint64_t *scratch_bytes) {
    const uint32_t g = geometry_grid(true, n, MZ_ZS_WAVES_PER_CU, grid);
    if (scratch_bytes) *scratch_bytes = (uint64_t)g * MZ_ZS_SCRATCH_BYTES;
}

int32_t mzhip_zstd_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                         const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, uint32_t *d_out_len,
                         uint32_t *d_in_used, uint32_t *d_crc, int32_t *d_status, void *stream) {
    static const Kernel<WaveScratchArgs> k = MZ_KERNEL(k_zstd_batch);
    WaveScratchArgs a{};
    return wave_per_entry_batch(k, a, MZ_ZS_WAVES_PER_CU, MZ_ZS_SCRATCH_BYTES, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n,
                                d_out_len, d_in_used, d_crc, d_status, stream);
}

/* bzip2 encode: the sort of a block's rotations needs, per resident wave and per symbol the scratch holds, two rotation
 * orders and two rank arrays of 4 bytes each (prefix doubling reads one pair and writes the other; the second rank array
 * is the scatter's fill counts, the first holds the 16-bit symbols once the sort is done) and the symbol itself: 17 bytes,
 * and 18 048 bytes of selectors.  The scratch holds C = min(100000 * level, max_in_len + max_in_len / 4 + 1) symbols, rounded
 * up to 64 (MZ_BZE_CAP_SYMS): MZ_BZE_SCRATCH_BYTES(C) = 17 C + 18 048, rounded up to 256 -- 1 411 840 bytes for entries of
 * 64 KiB at any level (C = 81 984), 15 318 784 for entries of 900 000 bytes and more at level 9 (C = 900 032).
 * 4 single-wave workgroups per CU, one per SIMD: the sort waits for scattered loads, so more waves would hide more of it
 * -- LDS (27.8 KiB per wave) would allow 5 -- but every further wave per CU costs 3.9 GB of scratch on a 256-CU device at
 * level 9; 4 per CU is 15.7 GB for a full grid there and 1.4 GB for 64 KiB entries.  grid = min(n, resident): a small
 * batch costs a small scratch. */
#define MZ_BZE_WAVES_PER_CU 4u

uint64_t mzhip_bzip2_encode_bound(uint32_t in_len, int32_t level) {
    const uint64_t digit = MZ_BZE_LEVEL(level);
    return digit ? MZ_BZE_BOUND(in_len, digit) : 0u;
}

void mzhip_bzip2_encode_launch_geometry(uint32_t n, uint32_t max_in_len, int32_t level, uint32_t *grid, uint64_t *scratch_bytes) {
    const uint32_t digit = MZ_BZE_LEVEL(level);
    const uint32_t g = geometry_grid(digit != 0u, n, MZ_BZE_WAVES_PER_CU, grid);
    if (scratch_bytes) *scratch_bytes = (uint64_t)g * MZ_BZE_SCRATCH_BYTES(MZ_BZE_CAP_SYMS(max_in_len, digit ? digit : 1u));
}

int32_t mzhip_bzip2_encode_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t max_in_len,
                                 void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, int32_t level,
                                 uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status, void *stream) {
    const uint32_t digit = MZ_BZE_LEVEL(level);
    if (!digit) {
        snprintf(g_err, sizeof(g_err), "mzhip_bzip2_encode_batch: level %d is not 1 .. 9 or -1", (int)level);
        return -102; /* MZ_PARAM_ERROR */
    }
    static const Kernel<Bzip2EncArgs> k = MZ_KERNEL(k_bzip2_encode_batch);
    Bzip2EncArgs a{};
    a.level = digit;
    a.cap_syms = MZ_BZE_CAP_SYMS(max_in_len, digit);
    a.scratch_stride = MZ_BZE_SCRATCH_BYTES(a.cap_syms);
    return wave_per_entry_batch(k, a, MZ_BZE_WAVES_PER_CU, (size_t)a.scratch_stride, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n,
                                d_out_len, nullptr /* an encoder takes all of its input */, d_crc, d_status, stream);
}

int32_t mzhip_sha_batch(const void *d_buf, const uint64_t *d_off, const uint32_t *d_len, uint32_t n, uint32_t algorithm,
                        void *d_digest, void *stream) {
    /* by algorithm - 20 (mz.h:127-135 defines no 21) */
    static const Kernel<ShaArgs> k[6] = {MZ_KERNEL(k_sha_batch<20>), {nullptr, nullptr},       MZ_KERNEL(k_sha_batch<22>),
                                         MZ_KERNEL(k_sha_batch<23>), MZ_KERNEL(k_sha_batch<24>), MZ_KERNEL(k_sha_batch<25>)};
    if (algorithm < 20 || algorithm > 25 || !k[algorithm - 20].fn) return MZHIP_STATUS_UNSUPPORTED;
    if (n == 0) return 0;
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    ShaArgs a{};
    a.buf = (const uint8_t *)d_buf;
    a.off = d_off;
    a.len = d_len;
    a.n = n;
    a.algorithm = algorithm;
    a.digest = (uint8_t *)d_digest;
    hipLaunchKernelGGL(k[algorithm - 20].fn, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int32_t mzhip_pkcrypt_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                            const uint64_t *d_out_off, uint32_t n, const uint8_t *password, uint32_t password_len,
                            const uint32_t *d_verify, uint32_t *d_out_len, int32_t *d_status, void *stream) {
    return pkcrypt_batch(k_pkcrypt_batch, d_in, d_in_off, d_in_len, d_out, d_out_off, n, password, password_len, d_verify, nullptr,
                         d_out_len, d_status, stream);
}

int32_t mzhip_wzaes_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, const uint8_t *d_strength,
                          void *d_out, const uint64_t *d_out_off, uint32_t n, const uint8_t *password, uint32_t password_len,
                          uint32_t *d_out_len, int32_t *d_status, void *stream) {
    static const Kernel<WzaesArgs> k[3] = {MZ_KERNEL(k_wzaes_keys), MZ_KERNEL(k_wzaes_ctr), MZ_KERNEL(k_wzaes_auth)};
    return wzaes_batch(k, d_in, d_in_off, d_in_len, d_strength, nullptr, d_out, d_out_off, n, password, password_len, d_out_len, d_status, stream);
}

int32_t mzhip_pkcrypt_encrypt_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                                    const uint64_t *d_out_off, uint32_t n, const uint8_t *password, uint32_t password_len,
                                    const uint32_t *d_verify, const uint8_t *d_header, uint32_t *d_out_len, int32_t *d_status,
                                    void *stream) {
    return pkcrypt_batch(k_pkcrypt_enc_batch, d_in, d_in_off, d_in_len, d_out, d_out_off, n, password, password_len, d_verify, d_header,
                         d_out_len, d_status, stream);
}

int32_t mzhip_wzaes_encrypt_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, const uint8_t *d_strength,
                                  const uint8_t *d_salt, void *d_out, const uint64_t *d_out_off, uint32_t n, const uint8_t *password,
                                  uint32_t password_len, uint32_t *d_out_len, int32_t *d_status, void *stream) {
    static const Kernel<WzaesArgs> k[3] = {MZ_KERNEL(k_wzaes_enc_keys), MZ_KERNEL(k_wzaes_enc_ctr), MZ_KERNEL(k_wzaes_enc_auth)};
    return wzaes_batch(k, d_in, d_in_off, d_in_len, d_strength, d_salt, d_out, d_out_off, n, password, password_len, d_out_len, d_status, stream);
}

int32_t mzhip_deflate_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                            const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_final, uint32_t n,
                            uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status, void *stream) {
    return mzhip_deflate_batch_level(d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_final, n, 1, 15, d_out_len, d_crc,
                                     d_status, stream);
}

int32_t mzhip_deflate_batch_level(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, void *d_out,
                                  const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_final, uint32_t n,
                                  int32_t level, int32_t window_log2, uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status,
                                  void *stream) {
    return deflate_batch_launch(d_in, d_in_off, d_in_len, nullptr, d_out, d_out_off, d_out_cap, d_final, n, level, window_log2, d_out_len,
                                d_crc, d_status, stream);
}
} // extern "C"
int32_t mzh::deflate_batch_launch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_warm, void *d_out,
                                  const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_final, uint32_t n,
                                  int32_t level, int32_t window_log2, uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status,
                                  void *stream) {
    if (n == 0) return 0;
    if (window_log2 < 9 || window_log2 > 15) return MZHIP_STATUS_UNSUPPORTED;
    Launch L;
    int32_t rc = L.begin(stream);
    if (rc) return rc;
    DeviceCtx *c = L.c;
    hipStream_t s = L.s;
    DeflateArgs a{};
    set_fields(a, c, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, nullptr /* an encoder takes all of its input */, d_crc, d_status);
    a.final_flag = d_final;
    a.warm = d_warm;
    a.counter = L.head.p;
    /* compression classes (mz_strm_zlib.c:87 hands `level` to deflateInit2): 0-3 fast = one candidate per hash bucket,
     * everything else (4-9, and -1 = Z_DEFAULT_COMPRESSION) = MZ_DEF_WAYS_BEST candidates + a two-position lazy rule */
    a.ways = (level >= 0 && level <= 3) ? 1u : MZ_DEF_WAYS_BEST;
    /* the default class needs 134 KiB of dynamic LDS per workgroup: a device (or runtime) that does not grant it gets the
     * one-candidate class -- a valid stream with a worse ratio, not a launch error */
    a.parse = (a.ways > 1u && level >= 7) ? 1u : 0u; /* levels 7-9 pay for ratio as they do in zlib */
    {
        const size_t big = MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * (MZ_DEF_LDS_STRIDE + MZ_DEF_XHEAD_BYTES);
        if (a.ways > 1u && !(a.parse ? big_lds_ok(c->big_lds_deflate_cost, (const void *)k_deflate_cost_batch, big)
                                     : big_lds_ok(c->big_lds_deflate, (const void *)k_deflate_batch, big))) {
            a.ways = 1u;
            a.parse = 0u;
        }
    }
    a.max_dist = (1u << window_log2) - 262u; /* zlib's MAX_DIST(s) = w_size - MIN_LOOKAHEAD */
    const size_t lds = MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * (MZ_DEF_LDS_STRIDE + (a.ways > 1u ? MZ_DEF_XHEAD_BYTES : 0));
#ifndef MZ_DEF_WGS
#define MZ_DEF_WGS 4u /* workgroups of the fast class per CU (measurement builds: 1, 2 -- traffic against residency, profiles/r6/README.md K4) */
#endif
    /* 38.3 / 134 KiB LDS per workgroup -> 4 / 1 per CU */
    const uint32_t grid = resident_grid((n + MZ_WAVES_PER_WG - 1) / MZ_WAVES_PER_WG, (uint32_t)c->cu_count * (a.ways > 1u ? 1u : MZ_DEF_WGS));
    ScratchLease sc; /* one token block per resident wave */
    rc = sc.get(&c->scratch, (size_t)grid * MZ_WAVES_PER_WG * MZ_DEF_BLOCK * sizeof(uint32_t), s);
    if (rc) return rc;
    a.tok = (uint32_t *)sc.p;
    if (a.parse) hipLaunchKernelGGL(k_deflate_cost_batch, dim3(grid), dim3(MZ_WAVES_PER_WG * 64), lds, s, a);
    else hipLaunchKernelGGL(k_deflate_batch, dim3(grid), dim3(MZ_WAVES_PER_WG * 64), lds, s, a);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess && a.ways > 1u) { /* the device does not take 134 KiB of LDS per workgroup after all */
        (a.parse ? c->big_lds_deflate_cost : c->big_lds_deflate).store(-1, std::memory_order_release);
        a.ways = 1u;
        a.parse = 0u;
        hipLaunchKernelGGL(k_deflate_batch, dim3(grid), dim3(MZ_WAVES_PER_WG * 64), MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * MZ_DEF_LDS_STRIDE, s, a);
        le = hipGetLastError();
    }
    return launched("k_deflate_batch", le, sc);
}

namespace {
/* K6's parse, shared by the batch, the segment and the .xz launchers: the chain pass over every stream of more than one
 * block (a.links set: `chain_waves` resident waves, one stream at a time each), then the block parse, one wave per 64 KiB
 * block.  The default class wants 128 KiB of dynamic LDS per workgroup (four hash ways per wave); a device or runtime that
 * does not grant it gets the one-candidate class -- a valid stream with a worse ratio, not a launch error. */
void launch_lz_parse(DeviceCtx *c, hipStream_t s, LzmaEncArgs &a, uint32_t chain_waves) {
    if (a.links && chain_waves) hipLaunchKernelGGL(k_lz_chain_batch, dim3(chain_waves), dim3(64), 0, s, a);
    const size_t items = (size_t)a.n * a.maxb;
    const uint32_t wgs = (uint32_t)((items + MZ_WAVES_PER_WG - 1) / MZ_WAVES_PER_WG);
    const size_t lds = MZ_WAVES_PER_WG * (sizeof(mz_lz_tok_lds) + (a.ways > 1u ? MZ_DEF_XHEAD_BYTES : 0));
    const uint32_t cus = (uint32_t)c->cu_count; /* 128 KiB (32 KiB) of LDS per workgroup: 1 (4) per CU */
    hipLaunchKernelGGL(k_lz_tokenize_batch, dim3(resident_grid(wgs, cus * (a.ways > 1u ? 1u : 4u))), dim3(MZ_WAVES_PER_WG * 64), lds, s, a);
    if (a.ways > 1u && hipGetLastError() != hipSuccess) { /* 128 KiB of LDS per workgroup refused after all */
        c->big_lds_tok.store(-1, std::memory_order_release);
        a.ways = 1u;
        hipLaunchKernelGGL(k_lz_tokenize_batch, dim3(resident_grid(wgs, cus * 4u)), dim3(MZ_WAVES_PER_WG * 64),
                           MZ_WAVES_PER_WG * sizeof(mz_lz_tok_lds), s, a);
    }
}
/* preset (mz_strm_lzma.c:81 hands COMPRESS_LEVEL to lzma_lzma_preset): 0-3 -> one hash candidate per position, 4-9 and
 * the default (-1 = 6) -> MZ_DEF_WAYS_BEST candidates + the two-position lazy rule, as K4's classes -- where the device
 * grants the tokenizer its 128 KiB of dynamic LDS per workgroup, the one-candidate class where it does not */
void set_lz_class(DeviceCtx *c, LzmaEncArgs &a, int32_t preset) {
    a.ways = (preset >= 0 && preset <= 3) ? 1u : MZ_DEF_WAYS_BEST;
    a.far_depth = MZ_LZE_DEPTH_FOR_PRESET(preset);
    if (a.ways > 1u && !big_lds_ok(c->big_lds_tok, (const void *)k_lz_tokenize_batch, MZ_WAVES_PER_WG * (sizeof(mz_lz_tok_lds) + MZ_DEF_XHEAD_BYTES)))
        a.ways = 1u;
}
/* The scratch of K6's parse, laid out in one place for every launcher of it: 4 bytes of token per input position of the
 * largest entry, for every entry (n x maxb blocks); when an entry has more than one block, as much again for the chain
 * pass's links and 1 MiB of table per resident wave of that pass; a token count per block; three work counters; and, behind
 * the next 256-byte boundary, `coder_bytes` for the kernel that codes the tokens (0: it needs none, and no padding). */
struct LzScratch {
    uint32_t chain_waves; /* waves of the chain pass, 0: no entry of more than one block */
    size_t items, tok_words, link_words, coder_off, bytes;
    /* the parse's pointers into a lease of `bytes` at p; the counters are zeroed and the parse is queued */
    int32_t parse(DeviceCtx *c, hipStream_t s, LzmaEncArgs &a, void *p) const {
        a.tok = (uint32_t *)p;
        a.links = chain_waves ? a.tok + tok_words : nullptr;
        a.chain_head = chain_waves ? a.links + tok_words : nullptr;
        a.ntok = a.tok + tok_words + link_words;
        a.counter = a.ntok + items;
        HIP_TRY(hipMemsetAsync(a.counter, 0, 3 * sizeof(uint32_t), s));
        launch_lz_parse(c, s, a, chain_waves);
        return 0;
    }
};
LzScratch lz_scratch(uint32_t n, uint32_t maxb, size_t coder_bytes) {
    LzScratch l{};
    l.items = (size_t)n * maxb;
    l.tok_words = l.items * MZ_DEF_BLOCK;
    l.chain_waves = maxb > 1u ? resident_grid(n, MZ_LZE_CHAIN_WAVES) : 0u;
    l.link_words = l.chain_waves ? l.tok_words + ((size_t)l.chain_waves << MZ_LZE_FAR_HBITS) : 0u;
    const size_t parse_bytes = (l.tok_words + l.link_words + l.items + 3u) * sizeof(uint32_t);
    l.coder_off = (parse_bytes + 255u) & ~(size_t)255u;
    l.bytes = coder_bytes ? l.coder_off + coder_bytes : parse_bytes;
    return l;
}
uint32_t lz_blocks(uint32_t in_len) { return in_len ? (in_len + MZ_DEF_BLOCK - 1) / MZ_DEF_BLOCK : 1u; }
/* ONE stream of `maxb` blocks for the host-buffer writers, parsed: entry 0's words are the meta block's at `base` (offsets
 * from there), `tok` has lz_scratch(1, maxb, 0).bytes of room; skip_blocks of history in front are linked (the segment's
 * links point into them), not parsed */
template <class Meta>
int32_t lz_parse_one_stream(DeviceCtx *c, hipStream_t s, LzmaEncArgs &a, uint8_t *base, Meta *dm, uint32_t maxb, uint32_t skip_blocks,
                            int32_t preset, uint32_t *tok) {
    set_fields(a, c, base, &dm->in_off, &dm->in_len, base, &dm->out_off, &dm->out_cap, 1, &dm->out_len, nullptr, &dm->crc, &dm->status);
    a.maxb = maxb;
    set_lz_class(c, a, preset);
    a.skip_blocks = skip_blocks;
    return lz_scratch(1, maxb, 0).parse(c, s, a, tok);
}
} // namespace
extern "C" {

int32_t mzhip_lzma_encode_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t max_in_len,
                                void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_mode,
                                uint32_t n, uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status, void *stream) {
    return mzhip_lzma_encode_batch_preset(d_in, d_in_off, d_in_len, max_in_len, d_out, d_out_off, d_out_cap, d_mode, n, 1,
                                          d_out_len, d_crc, d_status, stream);
}

int32_t mzhip_lzma_encode_batch_preset(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t max_in_len,
                                       void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, const uint8_t *d_mode,
                                       uint32_t n, int32_t preset, uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status,
                                       void *stream) {
    if (n == 0) return 0;
    Launch L;
    int32_t rc = L.begin(stream, false); /* (three work counters of its own, in the scratch) */
    if (rc) return rc;
    DeviceCtx *c = L.c;
    hipStream_t s = L.s;
    LzmaEncArgs a{};
    set_fields(a, c, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, nullptr /* an encoder takes all of its input */, d_crc, d_status);
    a.mode = d_mode;
    a.maxb = lz_blocks(max_in_len);
    set_lz_class(c, a, preset);
    const LzScratch lay = lz_scratch(n, a.maxb, 0);
    ScratchLease sc;
    rc = sc.get(&c->scratch, lay.bytes, s);
    if (rc) return rc;
    rc = lay.parse(c, s, a, sc.p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lzma_rc_encode_batch, dim3(resident_grid(n, (uint32_t)c->cu_count * 9u)), dim3(64), 0, s, a); /* 17 KiB LDS per single-wave workgroup */
    return launched("k_lzma_rc_encode_batch", hipGetLastError(), sc);
}

/* zstd encode: K6's parse (token scratch as for LZMA: 4 bytes per input position of the largest entry for every entry, as
 * much again and the chain pass's tables when an entry has more than one block), then one wave per entry.  That wave owns
 * MZ_ZSE_SCRATCH_BYTES = 263 168 of the scratch: the block's literals, its sequence records and the staged body.  8
 * single-wave workgroups per CU, two per SIMD (15.6 KiB of LDS each would allow 10; 253 VGPRs allow 8): the FSE walk is a chain of dependent LDS
 * reads, so a wave mostly waits.  A full grid on a 256-CU device holds 514 MiB of it.  grid = min(n, resident). */
#define MZ_ZSE_WAVES_PER_CU 8u

uint64_t mzhip_zstd_encode_bound(uint32_t in_len) { return MZ_ZSE_BOUND(in_len); }

void mzhip_zstd_encode_launch_geometry(uint32_t n, uint32_t max_in_len, int32_t level, uint32_t *grid, uint64_t *scratch_bytes) {
    const uint32_t g = geometry_grid(n && MZ_ZSE_LEVEL_OK(level), n, MZ_ZSE_WAVES_PER_CU, grid);
    if (scratch_bytes) *scratch_bytes = g ? lz_scratch(n, lz_blocks(max_in_len), (size_t)g * MZ_ZSE_SCRATCH_BYTES).bytes : 0u;
}

int32_t mzhip_zstd_encode_batch(const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, uint32_t max_in_len,
                                void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_cap, uint32_t n, int32_t level,
                                uint32_t flags, uint32_t *d_out_len, uint32_t *d_crc, int32_t *d_status, void *stream) {
    if (!MZ_ZSE_LEVEL_OK(level)) {
        snprintf(g_err, sizeof(g_err), "mzhip_zstd_encode_batch: level %d is not -1 .. 22", (int)level);
        return -102; /* MZ_PARAM_ERROR */
    }
    if (n == 0) return 0;
    Launch L;
    int32_t rc = L.begin(stream, false); /* (three work counters of its own, in the scratch) */
    if (rc) return rc;
    DeviceCtx *c = L.c;
    hipStream_t s = L.s;
    ZstdEncArgs z{};
    LzmaEncArgs &a = z.a;
    set_fields(a, c, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, n, d_out_len, nullptr /* an encoder takes all of its input */, d_crc, d_status);
    a.maxb = lz_blocks(max_in_len);
    set_lz_class(c, a, MZ_ZSE_PRESET(level));
    const uint32_t grid = wave_grid(c, n, MZ_ZSE_WAVES_PER_CU);
    const LzScratch lay = lz_scratch(n, a.maxb, (size_t)grid * MZ_ZSE_SCRATCH_BYTES);
    ScratchLease sc;
    rc = sc.get(&c->scratch, lay.bytes, s);
    if (rc) return rc;
    z.scratch = (uint8_t *)sc.p + lay.coder_off;
    z.flags = flags;
    rc = lay.parse(c, s, a, sc.p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_zstd_encode_batch, dim3(grid), dim3(64), 0, s, z);
    return launched("k_zstd_encode_batch", hipGetLastError(), sc);
}

} // extern "C"

// ---- one window of one large entry, a wave per DEFLATE block (the orchestration: inflate_parallel.inc)
#include "inflate_parallel.inc"
namespace {
// the header search of a window: 32 bit offsets per lane (which = 0), or the kernel it replaced, one offset per lane (1: tests)
hipError_t launch_find(const DeviceCtx *c, const ParFindArgs &a, hipStream_t s, int which) {
    const uint64_t per_wg = which ? 256u : 256u * 32u;
    const uint64_t want = ((uint64_t)(a.b1 - a.b0) + per_wg - 1u) / per_wg;
    const uint32_t grid = resident_grid(want ? want : 1u, (uint64_t)c->cu_count * 32u);
    if (which)
        hipLaunchKernelGGL(k_find_blocks_lane, dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_find_blocks, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}
// ... and the headers behind the candidates read to their end, a lane each: out[] / *out_count = the ones a decoder would get past
hipError_t launch_check(const DeviceCtx *c, const ParFindArgs &f, uint32_t *out, uint32_t *out_count, hipStream_t s) {
    ParCheckArgs a{};
    a.in = f.in;
    a.in_len = f.in_len;
    a.cands = f.cands;
    a.count = f.count;
    a.cap = f.cap;
    a.out = out;
    a.out_count = out_count;
    /* (the count is on the device: a grid-stride loop over it) */
    hipLaunchKernelGGL(k_check_headers, dim3(resident_grid((f.cap + 255u) / 256u, (uint32_t)c->cu_count * 4u)), dim3(256), 0, s, a);
    return hipGetLastError();
}
int header_check_on() { // MZHIP_HEADER_CHECK=0: every candidate of the search goes to the counting pass, as before round 6 (A/B)
    static const int on = [] {
        const char *e = getenv("MZHIP_HEADER_CHECK");
        return (e && e[0] == '0') ? 0 : 1;
    }();
    return on;
}
struct DevParBackend {
    DeviceCtx *c;
    hipStream_t s;
    const uint8_t *d_in;
    uint32_t in_len;
    uint8_t *d_buf;
    uint32_t *d_ptr, *d_cands, *d_bits, *d_pos, *d_res, *d_count; // d_count: [0] candidates found, [1] "a pointer moved"
    uint32_t cap;
    int wgs_per_cu;
    double t_find = 0, t_parse[3] = {0, 0, 0}, t_resolve = 0; // MZHIP_PAR_TRACE=1: seconds per step (each ends in a blocking copy)
    uint32_t n_parse[3] = {0, 0, 0};
    uint32_t n_found = 0; // offsets the search passed on (before the header check)
    static double now() {
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
    }
    int32_t find(uint32_t b0, uint32_t b1, std::vector<uint32_t> &cands) {
        const double t0 = now();
        const int32_t rc = find_(b0, b1, cands);
        t_find += now() - t0;
        return rc;
    }
    int32_t parse(uint32_t mode, const uint32_t *bits, const uint32_t *pos, uint32_t n, MzParBlock *res) {
        const double t0 = now();
        const int32_t rc = parse_(mode, bits, pos, n, res);
        t_parse[mode & 3u] += now() - t0;
        n_parse[mode & 3u] += n;
        return rc;
    }
    int32_t resolve(uint32_t hist, uint32_t total, uint32_t *rounds) {
        const double t0 = now();
        const int32_t rc = resolve_(hist, total, rounds);
        if (rc == 0) (void)hipStreamSynchronize(s);
        t_resolve += now() - t0;
        return rc;
    }
    int32_t find_(uint32_t b0, uint32_t b1, std::vector<uint32_t> &cands) {
        HIP_TRY(hipMemsetAsync(d_count, 0, 16, s)); /* [0] found, [1] "a pointer moved" (resolve), [2] kept by the header check */
        ParFindArgs a{};
        a.in = d_in;
        a.in_len = in_len;
        a.b0 = b0;
        a.b1 = b1;
        a.cands = d_cands;
        a.cap = cap;
        a.count = d_count;
        HIP_TRY(launch_find(c, a, s, 0));
        const int check = header_check_on();
        if (check) HIP_TRY(launch_check(c, a, d_bits, d_count + 2, s)); /* (d_bits: the counting pass fills it only after this) */
        uint32_t nn[4] = {0, 0, 0, 0};
        HIP_TRY(mz_d2h_on(s, nn, d_count, 16));
        n_found += nn[0];
        if (nn[0] > cap) return MZHIP_PAR_BAIL; /* (more candidates than anything but an adversary's stream holds: stream order) */
        const uint32_t n = check ? nn[2] : nn[0];
        cands.resize(n);
        if (n) HIP_TRY(mz_d2h_on(s, cands.data(), check ? d_bits : d_cands, (size_t)n * 4));
        return 0;
    }
    int32_t parse_(uint32_t mode, const uint32_t *bits, const uint32_t *pos, uint32_t n, MzParBlock *res) {
        if (n > cap + 1u) return MZHIP_PAR_BAIL;
        HIP_TRY(mz_h2d_on(s, d_bits, bits, (size_t)n * 4));
        HIP_TRY(mz_h2d_on(s, d_pos, pos, (size_t)n * 4));
        ParBlocksArgs a{};
        a.in = d_in;
        a.in_len = in_len;
        a.out = d_buf;
        a.ptr = d_ptr;
        a.bits = d_bits;
        a.pos = d_pos;
        a.n = n;
        a.mode = mode;
        a.res = d_res;
        a.tabs = c->d_tabs;
        CounterLease head;
        int32_t rc = head.get(&c->counters, s);
        if (rc) return rc;
        a.counter = head.p;
        const uint32_t need = (n + MZ_WAVES_PER_WG - 1) / MZ_WAVES_PER_WG;
        const uint32_t grid = resident_grid(need ? need : 1u, (uint32_t)(c->cu_count * wgs_per_cu));
        ScratchLease sc;
        rc = sc.get(&c->scratch, (size_t)grid * MZ_WAVES_PER_WG * MZ_REC_BYTES + 1024, s);
        if (rc) return rc;
        a.rec = (uint8_t *)sc.p;
        hipLaunchKernelGGL(k_inflate_blocks, dim3(grid), dim3(MZ_WAVES_PER_WG * 64), MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * MZ_LDS_STRIDE, s, a);
        rc = launched("k_inflate_blocks", hipGetLastError(), sc);
        if (rc) return rc;
        static_assert(sizeof(MzParBlock) == 16, "four words per candidate, as mz_inflate_one_block writes them");
        HIP_TRY(mz_d2h_on(s, res, d_res, (size_t)n * 16));
        return 0;
    }
    int32_t resolve_(uint32_t hist, uint32_t total, uint32_t *rounds) {
        ParJumpArgs a{};
        a.out = d_buf;
        a.ptr = d_ptr;
        a.hist = hist;
        a.total = total;
        a.changed = d_count + 1;
        const uint64_t want = ((uint64_t)(total - hist) + 255u) / 256u;
        const uint32_t grid = resident_grid(want ? want : 1u, (uint64_t)c->cu_count * 32u);
        for (uint32_t r = 0; r < 40u; r++) { /* (2^40 > any chain inside a 2 GiB window) */
            HIP_TRY(hipMemsetAsync(d_count + 1, 0, 4, s));
            /* two rounds (of up to four links each) per look at the flag: the look is a round trip to the host */
            hipLaunchKernelGGL(k_ptr_jump, dim3(grid), dim3(256), 0, s, a);
            hipLaunchKernelGGL(k_ptr_jump, dim3(grid), dim3(256), 0, s, a);
            HIP_TRY(hipGetLastError());
            uint32_t changed = 0;
            HIP_TRY(mz_d2h_on(s, &changed, d_count + 1, 4));
            *rounds += 2;
            if (!changed) break;
        }
        hipLaunchKernelGGL(k_ptr_gather, dim3(grid), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
};
// one large entry where it lies (inflate_parallel.inc mz_large_entry): views of the entry's input and output, one scratch
// block for the source map and the candidates of the largest window
struct DevLargeBackend {
    DeviceCtx *c;
    hipStream_t s;
    const uint8_t *d_in;
    uint8_t *d_out;
    uint8_t *scratch; // [source map: 4 B x (MZ_LARGE_WINDOW + 32 KiB + 64)][cands][bits][pos][res][counters][serial meta]
    uint32_t cap;
    int wgs_per_cu;
    size_t o_cands, o_bits, o_pos, o_res, o_count, o_meta;
    double t_par = 0, t_serial = 0;
    int32_t window(uint32_t vbyte, uint32_t vlen, uint32_t obase, uint32_t buf_cap, uint32_t start_bit, uint32_t hist, MzParWindow *w) {
        const double t0 = DevParBackend::now();
        DevParBackend be;
        be.c = c;
        be.s = s;
        be.d_in = d_in + vbyte;
        be.in_len = vlen;
        be.d_buf = d_out + obase;
        be.d_ptr = (uint32_t *)scratch;
        be.d_cands = (uint32_t *)(scratch + o_cands);
        be.d_bits = (uint32_t *)(scratch + o_bits);
        be.d_pos = (uint32_t *)(scratch + o_pos);
        be.d_res = (uint32_t *)(scratch + o_res);
        be.d_count = (uint32_t *)(scratch + o_count);
        be.cap = cap;
        be.wgs_per_cu = wgs_per_cu;
        int32_t rc = mz_parallel_window(be, vlen, buf_cap, start_bit, hist, w);
        if (rc == MZHIP_PAR_BAIL) { /* (more candidates than the arrays hold: stream order for this window) */
            *w = MzParWindow();
            rc = 0;
        }
        t_par += DevParBackend::now() - t0;
        return rc;
    }
    int32_t serial(uint32_t vbyte, uint32_t vlen, uint32_t obase, uint32_t buf_cap, uint32_t hdr_bit, uint32_t bit, uint32_t hist, uint32_t flags,
                   MzSerialResult *o) {
        const double t0 = DevParBackend::now();
        struct Meta {
            uint64_t in_off, out_off;
            uint32_t in_len, out_cap, out_len, in_used, crc;
            int32_t status;
            mz_inflate_state rs, st;
        } m;
        memset(&m, 0, sizeof(m));
        m.in_len = vlen;
        m.out_cap = buf_cap;
        m.rs.hdr_bit = hdr_bit;
        m.rs.bit = bit;
        m.rs.out_pos = hist;
        m.rs.flags = flags;
        Meta *dm = (Meta *)(scratch + o_meta);
        HIP_TRY(mz_h2d_on(s, dm, &m, sizeof(m)));
        const int32_t rc = mzhip_inflate_resume_batch(d_in + vbyte, &dm->in_off, &dm->in_len, d_out + obase, &dm->out_off, &dm->out_cap, 1, &dm->out_len,
                                                      &dm->in_used, &dm->crc, &dm->status, (const mzhip_inflate_state *)&dm->rs,
                                                      (mzhip_inflate_state *)&dm->st, s);
        if (rc) return rc;
        HIP_TRY(mz_d2h_on(s, &m, dm, sizeof(m)));
        o->status = m.status;
        o->out_len = m.out_len;
        o->in_used = m.in_used;
        o->hdr_bit = m.st.hdr_bit;
        o->bit = m.st.bit;
        o->out_pos = m.st.out_pos;
        o->ok = m.st.flags & 1u;
        t_serial += DevParBackend::now() - t0;
        return 0;
    }
};
static int par_trace() { // MZHIP_PAR_TRACE=1: what every window and large entry cost, step by step, on stderr
    static const int on = [] {
        const char *e = getenv("MZHIP_PAR_TRACE");
        return (e && e[0] == '1') ? 1 : 0;
    }();
    return on;
}
static int par_wgs_per_cu() { /* resident workgroups per CU of k_inflate_blocks (asked once) */
    static std::atomic<int> s_wgs{0};
    int wgs = s_wgs.load(std::memory_order_relaxed);
    if (wgs == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_inflate_blocks, MZ_WAVES_PER_WG * 64,
                                                         MZ_CRC_TAB_BYTES + MZ_WAVES_PER_WG * MZ_LDS_STRIDE) != hipSuccess || nb <= 0) {
            (void)hipGetLastError();
            nb = 1;
        }
        s_wgs.store(wgs = nb, std::memory_order_relaxed);
    }
    return wgs;
}
} // namespace

extern "C" {

// One large raw-DEFLATE entry, device-resident, by a wave per block (include/mzhip.h).  Synchronous: the host steers the
// windows; everything is queued on `stream` and waited for there.
int32_t mzhip_inflate_large(const void *d_in, uint32_t in_len, void *d_out, uint32_t out_cap, uint32_t *out_len, uint32_t *in_used,
                            uint32_t *crc, int32_t *status, void *stream) {
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    DevLargeBackend be;
    be.c = c;
    be.s = s;
    be.d_in = (const uint8_t *)d_in;
    be.d_out = (uint8_t *)d_out;
    be.cap = MZ_LARGE_SHOW_MAX / 16u + 4096u;
    be.wgs_per_cu = par_wgs_per_cu();
    const size_t win = out_cap < MZ_LARGE_WINDOW ? out_cap : MZ_LARGE_WINDOW;
    const size_t map = ((win + 32768 + 64) * 4 + 255) & ~(size_t)255, arr = ((size_t)(be.cap + 4) * 4 + 255) & ~(size_t)255;
    const size_t ck_max = (size_t)out_cap / 65536u + 3;
    be.o_cands = map;
    be.o_bits = be.o_cands + arr;
    be.o_pos = be.o_bits + arr;
    be.o_res = be.o_pos + arr;
    be.o_count = be.o_res + arr * 4;
    be.o_meta = be.o_count + 256;
    const size_t o_ck = be.o_meta + 256, total = o_ck + ck_max * 16;
    ScratchLease sc;
    rc = sc.get(&c->scratch, total, s);
    if (rc) return rc;
    be.scratch = (uint8_t *)sc.p;
    MzLargeResult r;
    rc = mz_large_entry(be, in_len, out_cap, &r);
    uint32_t k = 0;
    if (!rc && crc && r.out_len) rc = window_checksums(be.d_out, 0, 0, r.out_len, &k, nullptr, be.scratch + o_ck, ck_max, s);
    const int trace = par_trace();
    if (trace)
        fprintf(stderr, "mzhip large entry: %u B in, %u B out, status %d; %u many-wave windows (%u blocks, %.2f ms), %u serial calls (%.2f ms)\n", in_len,
                r.out_len, r.status, r.par_windows, r.par_blocks, be.t_par * 1e3, r.serial_calls, be.t_serial * 1e3);
    const int32_t rr = sc.release();
    if (rc) return rc;
    if (rr) return rr;
    if (out_len) *out_len = r.out_len;
    if (in_used) *in_used = r.in_used;
    if (crc) *crc = k;
    if (status) *status = r.status;
    return 0;
}

} // extern "C"

// ---- one large Zstandard entry, a wave per block (the orchestration: zstd_parallel.inc)
#include "zstd_parallel.inc"
namespace {
struct DevZstdLargeBackend {
    DeviceCtx *c;
    hipStream_t s;
    const uint8_t *d_in;
    uint32_t in_len;
    uint8_t *d_out;
    uint32_t *d_map; // the source map of one window
    uint32_t map_n;
    uint32_t *d_recs, *d_frms, *d_hdr, *d_jobs, *d_res, *d_flag;
    uint32_t cap; // blocks the arrays hold
    double t_scan = 0, t_pass[3] = {0, 0, 0}, t_resolve = 0, t_xxh = 0; // MZHIP_PAR_TRACE=1: seconds per step (each ends in a blocking copy)
    int32_t scan(uint32_t blk_cap, std::vector<uint32_t> &recs, std::vector<uint32_t> &frms, uint32_t *hdr) {
        const double t0 = DevParBackend::now();
        if (blk_cap > cap) return -104;
        ZstdScanArgs a{};
        a.in = d_in;
        a.in_len = in_len;
        a.blk_cap = blk_cap;
        a.recs = d_recs;
        a.frms = d_frms;
        a.hdr = d_hdr;
        hipLaunchKernelGGL(k_zstd_scan, dim3(1), dim3(64), 0, s, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(mz_d2h_on(s, hdr, d_hdr, MZ_ZSP_HDR_WORDS * 4));
        const uint32_t nb = hdr[MZ_ZSP_H_NBLK], nf = hdr[MZ_ZSP_H_NFRM];
        if (nb > blk_cap || nf > blk_cap) return -104;
        recs.resize((size_t)nb * MZ_ZSP_REC_WORDS);
        frms.resize((size_t)nf * MZ_ZSP_FRM_WORDS);
        if (nb && hdr[MZ_ZSP_H_STOP] == 0) HIP_TRY(mz_d2h_on(s, recs.data(), d_recs, recs.size() * 4));
        if (nf && hdr[MZ_ZSP_H_STOP] == 0) HIP_TRY(mz_d2h_on(s, frms.data(), d_frms, frms.size() * 4));
        t_scan += DevParBackend::now() - t0;
        return 0;
    }
    int32_t blocks(uint32_t mode, const uint32_t *jobs, uint32_t n, uint32_t bias, uint32_t *res) {
        const double t0 = DevParBackend::now();
        if (n == 0 || n > cap) return -104;
        if (mode == 2u && jobs[(size_t)(n - 1u) * MZ_ZSP_JOB_WORDS + MZ_ZSP_J_END] - bias > map_n) return -104;
        HIP_TRY(mz_h2d_on(s, d_jobs, jobs, (size_t)n * MZ_ZSP_JOB_WORDS * 4));
        ZstdBlocksArgs a{};
        a.in = d_in;
        a.in_len = in_len;
        a.out = d_out;
        a.ptr = (uint32_t *)((uintptr_t)d_map - 4u * (uintptr_t)bias);
        a.jobs = d_jobs;
        a.n = n;
        a.mode = mode;
        a.res = d_res;
        CounterLease head;
        int32_t rc = head.get(&c->counters, s);
        if (rc) return rc;
        a.counter = head.p;
        const uint32_t grid = wave_grid(c, n, MZ_ZS_WAVES_PER_CU);
        ScratchLease sc;
        rc = sc.get(&c->scratch, (size_t)grid * MZ_ZS_SCRATCH_BYTES, s);
        if (rc) return rc;
        a.scratch = (uint8_t *)sc.p;
        hipLaunchKernelGGL(k_zstd_blocks, dim3(grid), dim3(64), 0, s, a);
        rc = launched("k_zstd_blocks", hipGetLastError(), sc);
        if (rc) return rc;
        HIP_TRY(mz_d2h_on(s, res, d_res, (size_t)n * MZ_ZSP_RES_WORDS * 4));
        t_pass[mode & 3u] += DevParBackend::now() - t0;
        return 0;
    }
    // the DEFLATE path's kernels over a biased map: roots are literals and everything in front of the window
    int32_t resolve(uint32_t w0, uint32_t w1, uint32_t *rounds) {
        const double t0 = DevParBackend::now();
        if (w1 - w0 > map_n) return -104;
        ParJumpArgs a{};
        a.out = d_out;
        a.ptr = (uint32_t *)((uintptr_t)d_map - 4u * (uintptr_t)w0);
        a.hist = w0;
        a.total = w1;
        a.changed = d_flag;
        const uint64_t want = ((uint64_t)(w1 - w0) + 255u) / 256u;
        const uint32_t grid = resident_grid(want ? want : 1u, (uint64_t)c->cu_count * 32u);
        for (uint32_t r = 0; r < 40u; r++) {
            HIP_TRY(hipMemsetAsync(d_flag, 0, 4, s));
            hipLaunchKernelGGL(k_ptr_jump, dim3(grid), dim3(256), 0, s, a);
            hipLaunchKernelGGL(k_ptr_jump, dim3(grid), dim3(256), 0, s, a);
            HIP_TRY(hipGetLastError());
            uint32_t changed = 0;
            HIP_TRY(mz_d2h_on(s, &changed, d_flag, 4));
            *rounds += 2;
            if (!changed) break;
        }
        hipLaunchKernelGGL(k_ptr_gather, dim3(grid), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        t_resolve += DevParBackend::now() - t0;
        return 0;
    }
    int32_t xxh(const uint32_t *spans, uint32_t n, uint32_t *vals) { /* (the jobs and results of the passes are done with) */
        const double t0 = DevParBackend::now();
        if (n > cap) return -104;
        HIP_TRY(mz_h2d_on(s, d_jobs, spans, (size_t)n * 8));
        ZstdXxhArgs a{};
        a.out = d_out;
        a.spans = d_jobs;
        a.n = n;
        a.vals = d_res;
        hipLaunchKernelGGL(k_zstd_frame_xxh, dim3(resident_grid(n, (uint64_t)c->cu_count * 8u)), dim3(64), 0, s, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(mz_d2h_on(s, vals, d_res, (size_t)n * 4));
        t_xxh += DevParBackend::now() - t0;
        return 0;
    }
};
} // namespace

extern "C" {

// One large Zstandard entry, device-resident, by a wave per block (include/mzhip.h).  Synchronous: the host composes what
// crosses blocks; everything is queued on `stream` and waited for there.
int32_t mzhip_zstd_large(const void *d_in, uint32_t in_len, void *d_out, uint32_t out_cap, uint32_t window_bytes, uint32_t *out_len,
                         uint32_t *in_used, uint32_t *crc, int32_t *status, mzhip_zstd_large_stats *stats, void *stream) {
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t window = window_bytes ? window_bytes : MZ_LARGE_WINDOW;
    DevZstdLargeBackend be;
    be.c = c;
    be.s = s;
    be.d_in = (const uint8_t *)d_in;
    be.in_len = in_len;
    be.d_out = (uint8_t *)d_out;
    be.cap = in_len / 3u + 1u < MZ_ZSP_BLOCK_CAP ? in_len / 3u + 1u : MZ_ZSP_BLOCK_CAP;
    be.map_n = window > MZ_ZS_BLOCK_MAX ? window : MZ_ZS_BLOCK_MAX;
    if (be.map_n > out_cap) be.map_n = out_cap;
    const auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t ck_max = (size_t)out_cap / 65536u + 3;
    const size_t o_recs = pad((size_t)be.map_n * 4 + 64), o_frms = o_recs + pad((size_t)be.cap * MZ_ZSP_REC_WORDS * 4);
    const size_t o_hdr = o_frms + pad(((size_t)be.cap + 1u) * MZ_ZSP_FRM_WORDS * 4), o_jobs = o_hdr + 256;
    const size_t o_res = o_jobs + pad((size_t)be.cap * MZ_ZSP_JOB_WORDS * 4), o_meta = o_res + pad((size_t)be.cap * MZ_ZSP_RES_WORDS * 4);
    const size_t o_ck = o_meta + 256, total = o_ck + ck_max * 16;
    ScratchLease sc;
    rc = sc.get(&c->scratch, total, s);
    MzZsLarge r;
    uint32_t k = 0, ol = 0, iu = 0;
    int32_t st = 0;
    double t_crc = 0, t_one = 0;
    if (rc) { /* no room for the map and the arrays: the one-wave reader needs neither */
        r.fallback = 3u;
        (void)hipGetLastError();
    } else {
        uint8_t *base = (uint8_t *)sc.p;
        be.d_map = (uint32_t *)base;
        be.d_recs = (uint32_t *)(base + o_recs);
        be.d_frms = (uint32_t *)(base + o_frms);
        be.d_hdr = (uint32_t *)(base + o_hdr);
        be.d_flag = be.d_hdr + 16;
        be.d_jobs = (uint32_t *)(base + o_jobs);
        be.d_res = (uint32_t *)(base + o_res);
        rc = mz_zstd_large_entry(be, in_len, out_cap, window, &r);
        if (!rc && !r.fallback) {
            const double t0 = DevParBackend::now();
            ol = r.out_len;
            iu = in_len;
            if (crc && ol) rc = window_checksums(be.d_out, 0, 0, ol, &k, nullptr, base + o_ck, ck_max, s);
            t_crc = DevParBackend::now() - t0;
        }
        const int32_t rr = sc.release();
        if (!rc) rc = rr;
        if (rc) return rc;
    }
    if (r.fallback) { /* the whole entry through the one-wave kernel: its statuses, lengths and bytes */
        const double t0 = DevParBackend::now();
        struct Meta {
            uint64_t in_off, out_off;
            uint32_t in_len, out_cap, out_len, in_used, crc;
            int32_t status;
        } m;
        memset(&m, 0, sizeof(m));
        m.in_len = in_len;
        m.out_cap = out_cap;
        ScratchLease ms;
        rc = ms.get(&c->scratch, 256, s);
        if (rc) return rc;
        Meta *dm = (Meta *)ms.p;
        hipError_t e = mz_h2d_on(s, dm, &m, sizeof(m));
        if (e == hipSuccess) {
            rc = mzhip_zstd_batch(d_in, &dm->in_off, &dm->in_len, d_out, &dm->out_off, &dm->out_cap, 1, &dm->out_len, &dm->in_used, &dm->crc,
                                  &dm->status, s);
            if (!rc) e = mz_d2h_on(s, &m, dm, sizeof(m));
        }
        const int32_t rr = ms.release();
        if (e != hipSuccess) return fail("mzhip_zstd_large: the one-wave reader", e);
        if (!rc) rc = rr;
        if (rc) return rc;
        ol = m.out_len;
        iu = m.in_used;
        k = m.crc;
        st = m.status;
        t_one = DevParBackend::now() - t0;
    }
    if (par_trace())
        fprintf(stderr,
                "mzhip zstd large: %u B in, %u B out, status %d, fallback %u; %u windows, %u blocks (%u borrowed), %u rounds; ms: scan %.3f count %.3f "
                "emit %.3f resolve %.3f xxh64 %.3f crc %.3f one-wave %.3f\n",
                in_len, ol, st, r.fallback, r.windows, r.blocks, r.borrowed, r.rounds, be.t_scan * 1e3, be.t_pass[1] * 1e3, be.t_pass[2] * 1e3,
                be.t_resolve * 1e3, be.t_xxh * 1e3, t_crc * 1e3, t_one * 1e3);
    if (out_len) *out_len = ol;
    if (in_used) *in_used = iu;
    if (crc) *crc = k;
    if (status) *status = st;
    if (stats) {
        mzhip_zstd_large_stats v;
        const uint32_t n = stats->size < (uint32_t)sizeof(v) ? stats->size : (uint32_t)sizeof(v);
        v.size = n;
        v.windows = r.windows;
        v.blocks = r.blocks;
        v.borrowed = r.borrowed;
        v.rounds = r.rounds;
        v.fallback = r.fallback;
        memcpy(stats, &v, n);
    }
    return 0;
}

// (tests) the header search alone over host bytes placed `misalign` bytes behind a 16-byte boundary on the device: which = 0 the
// product's kernel, 1 the one-offset-per-lane kernel it replaced.  out[0 .. min(*n, cap)) = the candidates, in no order.
int32_t mzhip_find_blocks_host(const uint8_t *in, uint32_t in_len, uint32_t b0, uint32_t b1, int32_t which, uint32_t misalign, uint32_t *out,
                               uint32_t cap, uint32_t *n) {
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    if (!in || !out || !n || misalign > 15u || b1 < b0 || (uint64_t)b1 > 8ull * in_len) return -102;
    const size_t in_pad = ((size_t)in_len + misalign + 64 + 15) & ~(size_t)15;
    Staging sc;
    rc = sc.get(c, in_pad + 16 + 4 * (size_t)cap);
    if (rc) return rc;
    uint8_t *base = (uint8_t *)sc.p;
    HIP_TRY(hipMemsetAsync(base, 0, in_pad + 16, MZ_HOST_STREAM));
    HIP_TRY(mz_h2d(base + misalign, in, in_len));
    ParFindArgs a{};
    a.in = base + misalign;
    a.in_len = in_len;
    a.b0 = b0;
    a.b1 = b1;
    a.cands = (uint32_t *)(base + in_pad + 16);
    a.cap = cap;
    a.count = (uint32_t *)(base + in_pad);
    HIP_TRY(launch_find(c, a, MZ_HOST_STREAM, which == 1 ? 1 : 0));
    if (which == 2) { /* ... and the header check behind it (the candidates it keeps take the place of the search's) */
        uint32_t found = 0;
        HIP_TRY(mz_d2h(&found, a.count, 4));
        if (found > cap) return -104;
        Staging s2;
        rc = s2.get(c, 4 * (size_t)cap + 16);
        if (rc) return rc;
        uint32_t *kept = (uint32_t *)s2.p, *kept_n = kept + cap;
        HIP_TRY(hipMemsetAsync(kept_n, 0, 4, MZ_HOST_STREAM));
        HIP_TRY(launch_check(c, a, kept, kept_n, MZ_HOST_STREAM));
        HIP_TRY(mz_d2h(n, kept_n, 4));
        if (*n) HIP_TRY(mz_d2h(out, kept, (size_t)*n * 4));
        return 0;
    }
    HIP_TRY(mz_d2h(n, a.count, 4));
    const uint32_t k = *n < cap ? *n : cap;
    if (k) HIP_TRY(mz_d2h(out, a.cands, (size_t)k * 4));
    return 0;
}

int32_t mzhip_inflate_parallel_host(const uint8_t *in, uint32_t in_len, uint8_t *buf, uint32_t buf_cap,
                                    const mzhip_inflate_state *state_in, mzhip_inflate_state *state_out, uint32_t *out_len,
                                    uint32_t *blocks, uint32_t *ended, uint32_t *crc, uint32_t *adler, uint32_t seg_first, uint32_t seg_stride,
                                    uint32_t *seg_crc, uint32_t seg_cap, uint32_t *nseg) {
    const uint32_t hist = state_in ? state_in->out_pos : 0u;
    const double t_enter = DevParBackend::now();
    if (crc) *crc = 0u;
    if (adler) *adler = 1u;
    const uint32_t start = state_in && (state_in->flags & 1u) ? state_in->hdr_bit : 0u;
    if (nseg) *nseg = 0;
    if (blocks) *blocks = 0;
    if (ended) *ended = 0;
    if (out_len) *out_len = hist;
    if (state_in && (state_in->flags & 1u) && state_in->bit != state_in->hdr_bit) return 0; /* (inside a block: stream order) */
    if (hist > buf_cap) return -102;
    if (in_len >= (1u << 29) || in_len < 64u) return 0; /* (bit positions are 32 bits wide) */
    const int wgs = par_wgs_per_cu();
    // layout: [in][buf][source map: 4 B per byte of buf][candidates][bits][pos][results: 16 B each][two counters][segment arrays][checksum arrays]
    const size_t buf_room = ((size_t)buf_cap + 16 + 15) & ~(size_t)15;
    const uint32_t cap = in_len / 16u + 4096u;
    const size_t seg_max = (seg_stride && seg_crc) ? (size_t)buf_cap / seg_stride + 3 : 0;
    const size_t ck_max = (crc || adler) ? (size_t)buf_cap / 65536u + 3 : 0;
    StagedCall hc;
    const size_t o_in = hc.take((size_t)in_len + 64), o_buf = hc.take(buf_room), o_ptr = hc.take(4 * buf_room), o_cands = hc.take(4 * (size_t)(cap + 4)),
                 o_bits = hc.take(4 * (size_t)(cap + 4)), o_pos = hc.take(4 * (size_t)(cap + 4)), o_res = hc.take(16 * (size_t)(cap + 4)),
                 o_count = hc.take(16), o_seg = hc.take(seg_max * 16), o_ck = hc.take(ck_max * 16);
    int32_t rc = hc.begin();
    if (rc) return rc;
    DeviceCtx *c = hc.c;
    uint8_t *base = hc.at(0), *d_in = hc.at(o_in);
    HIP_TRY(mz_h2d(d_in, in, in_len));
    HIP_TRY(hipMemsetAsync(d_in + in_len, 0, (o_buf - o_in) - in_len, MZ_HOST_STREAM)); /* (up to the window) */
    if (hist) HIP_TRY(mz_h2d(hc.at(o_buf), buf, hist));
    DevParBackend be;
    be.c = c;
    be.s = MZ_HOST_STREAM;
    be.d_in = d_in;
    be.in_len = in_len;
    be.d_buf = hc.at(o_buf);
    be.d_ptr = (uint32_t *)hc.at(o_ptr);
    be.d_cands = (uint32_t *)hc.at(o_cands);
    be.d_bits = (uint32_t *)hc.at(o_bits);
    be.d_pos = (uint32_t *)hc.at(o_pos);
    be.d_res = (uint32_t *)hc.at(o_res);
    be.d_count = (uint32_t *)hc.at(o_count);
    be.cap = cap;
    be.wgs_per_cu = wgs;
    const int trace = par_trace();
    const double t0 = DevParBackend::now();
    if (trace) HIP_TRY(hipStreamSynchronize(MZ_HOST_STREAM));
    const double t1 = DevParBackend::now();
    MzParWindow w;
    rc = mz_parallel_window(be, in_len, buf_cap, start, hist, &w);
    const double t2 = DevParBackend::now();
    if (rc == 0 && w.blocks) {
        if (w.total > hist) HIP_TRY(mz_d2h(buf + hist, be.d_buf + hist, w.total - hist));
        const double t3 = DevParBackend::now();
        if (seg_max && w.total > hist) {
            rc = window_piece_crcs(base, o_buf, hist, w.total, seg_first, seg_stride, seg_crc, seg_cap, nseg, hc.at(o_seg), seg_max);
            if (rc) return rc;
        }
        if (ck_max) {
            rc = window_checksums(base, o_buf, hist, w.total, crc, adler, hc.at(o_ck), ck_max);
            if (rc) return rc;
        }
        if (trace)
            fprintf(stderr,
                    "mzhip parallel window: in %u B (from bit %u), %u candidates of %u offsets that looked like a header, %u blocks, %u B out, %u jump rounds | h2d %.2f ms, find %.2f, "
                    "count %.2f (%u waves), emit %.2f (%u), resolve %.2f, d2h %.2f, piece crcs %.2f; host: order %.2f, chain %.2f, set-up %.2f; %.2f ms so far\n",
                    in_len, start, w.candidates, be.n_found, w.blocks, w.total - hist, w.rounds, (t1 - t0) * 1e3, be.t_find * 1e3, be.t_parse[1] * 1e3,
                    be.n_parse[1], be.t_parse[2] * 1e3, be.n_parse[2], be.t_resolve * 1e3, (t3 - t2) * 1e3, (DevParBackend::now() - t3) * 1e3,
                    w.t_sort * 1e3, w.t_chain * 1e3, (t0 - t_enter) * 1e3, (DevParBackend::now() - t_enter) * 1e3);
    } else if (trace)
        fprintf(stderr, "mzhip parallel window: in %u B (from bit %u), %u candidates, nothing decoded (rc %d) | find %.2f ms, count %.2f (%u waves)\n",
                in_len, start, w.candidates, rc, be.t_find * 1e3, be.t_parse[1] * 1e3, be.n_parse[1]);
    if (rc == MZHIP_PAR_BAIL) return 0;
    if (rc) return rc;
    if (!w.blocks) return 0;
    if (blocks) *blocks = w.blocks;
    if (ended) *ended = w.ended;
    if (out_len) *out_len = w.total;
    if (state_out) {
        state_out->hdr_bit = state_out->bit = w.next_bit;
        state_out->out_pos = w.total;
        state_out->flags = 1u;
    }
    return 0;
}

uint32_t mzhip_lzma_model_bytes(void) { return (uint32_t)(MZ_LZMA_MODEL_U16 * sizeof(uint16_t)); }
uint32_t mzhip_lzma_encode_history_bytes(void) { return MZ_LZE_FAR_DICT; }

} // extern "C"

// One window of one stream through the resumable LZMA decoders, k_lzma_resume (ZIP method 14) and k_lzma2_run (an .xz block's
// chunk sequence): meta block, model, input and [dictionary so far | room for the window] in one staging buffer, one wave.
template <class State, class Args, class PubState>
static int32_t lzma_window_host(DeviceCtx *c, const Kernel<Args> &k, const uint8_t *in, uint32_t in_len, uint8_t *buf, uint32_t buf_cap,
                                const PubState *state_in, PubState *state_out, void *model, uint32_t *out_len, uint32_t *in_used) {
    static_assert(sizeof(PubState) == sizeof(State), "mzhip.h and the core header describe the same words");
    const uint32_t hist = state_in->out_pos;
    if (hist > buf_cap) return -102;
    struct Meta {
        State rs, st;
        uint32_t out_len, in_used;
        int32_t status;
    };
    HostCall<Meta> hc;
    hc.c = c;
    Meta &m = hc.m;
    memcpy(&m.rs, state_in, sizeof(m.rs));
    const size_t o_model = hc.take(MZ_LZMA_MODEL_U16 * sizeof(uint16_t)), o_in = hc.take((size_t)in_len + 16), o_buf = hc.take((size_t)buf_cap + 16);
    const int32_t rc = hc.begin();
    if (rc) return rc;
    uint8_t *d_model = hc.at(o_model), *d_in = hc.at(o_in), *d_buf = hc.at(o_buf);
    Meta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (state_in->flags & 1u) HIP_TRY(mz_h2d(d_model, model, MZ_LZMA_MODEL_U16 * sizeof(uint16_t)));
    if (in_len) HIP_TRY(mz_h2d(d_in, in, in_len));
    if (hist) HIP_TRY(mz_h2d(d_buf, buf, hist));
    Args a{d_in, in_len, d_buf, buf_cap, &dm->rs, state_out ? &dm->st : nullptr, (uint16_t *)d_model,
           &dm->out_len, &dm->in_used, &dm->status, c->d_tabs};
    if constexpr (std::is_same<Args, Lzma2RunArgs>::value) a.tab64 = c->d_tab64; /* the .xz block's CRC-64 */
    hipLaunchKernelGGL(k.fn, dim3(1), dim3(64), 0, MZ_HOST_STREAM, a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(k.name, le);
    HIP_TRY(hc.wait_fetch_meta());
    if (m.out_len > hist && m.out_len <= buf_cap) HIP_TRY(mz_d2h(buf + hist, d_buf + hist, m.out_len - hist));
    if (state_out) {
        memcpy(state_out, &m.st, sizeof(m.st));
        if (m.st.flags & 1u) HIP_TRY(mz_d2h(model, d_model, MZ_LZMA_MODEL_U16 * sizeof(uint16_t)));
    }
    give(out_len, m.out_len);
    give(in_used, m.in_used);
    return m.status;
}

extern "C" {

// One window of one ZIP method-14 payload (include/mzhip.h).  buf[0 .. state_in->out_pos) is the dictionary so far.
int32_t mzhip_lzma_resume_host(const uint8_t *in, uint32_t in_len, uint8_t *buf, uint32_t buf_cap, const mzhip_lzma_state *state_in,
                               mzhip_lzma_state *state_out, void *model, uint32_t *out_len, uint32_t *in_used) {
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    if (!model || !state_in) return -102; /* MZ_PARAM_ERROR */
    return lzma_window_host<mz_lzma_state, LzmaResumeArgs>(c, MZ_KERNEL(k_lzma_resume), in, in_len, buf, buf_cap, state_in, state_out, model,
                                                           out_len, in_used);
}

// One window of one .xz block's LZMA2 chunk sequence (include/mzhip.h).  buf[0 .. state_in->out_pos) is the dictionary so far.
int32_t mzhip_lzma2_run_host(const mzhip_lzma2_run_args *ap) {
    if (!ap || ap->size < offsetof(mzhip_lzma2_run_args, in_used) + sizeof(void *)) return -102; /* MZ_PARAM_ERROR */
    mzhip_lzma2_run_args g;
    memset(&g, 0, sizeof(g));
    memcpy(&g, ap, ap->size < sizeof(g) ? ap->size : sizeof(g));
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    if (!g.model || !g.state_in || !g.state_out || (!g.in && g.in_len) || !g.buf) return -102;
    return lzma_window_host<mz_lzma2_state, Lzma2RunArgs>(c, MZ_KERNEL(k_lzma2_run), g.in, g.in_len, g.buf, g.buf_cap, g.state_in, g.state_out,
                                                          g.model, g.out_len, g.in_used);
}

// One segment of one ZIP method-14 payload (include/mzhip.h): in = [skip_blocks x 64 KiB of the stream's previous bytes |
// the segment].
int32_t mzhip_lzma_encode_resume_host(const uint8_t *in, uint32_t in_len, uint32_t skip_blocks, uint32_t last, int32_t preset,
                                      const mzhip_lzma_enc_state *state_in, mzhip_lzma_enc_state *state_out, void *model,
                                      uint8_t *out, uint32_t out_cap, uint32_t *out_len) {
    static_assert(sizeof(mzhip_lzma_enc_state) == sizeof(mz_lzma_enc_state), "mzhip.h and lzma_enc_core.h describe the same sixteen words");
    struct Meta {
        mz_lzma_enc_state rs, st;
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, crc;
        int32_t status;
    };
    HostCall<Meta> hc;
    Meta &m = hc.m;
    int32_t rc = ctx_for_current(&hc.c);
    if (rc) return rc;
    if (!model || !state_in || (!last && !state_out) || (uint64_t)skip_blocks * MZ_DEF_BLOCK > in_len) return -102; /* MZ_PARAM_ERROR */
    const size_t model_bytes = ((LZ_NUM_PROBS + 1u) & ~1u) * sizeof(uint16_t);
    const uint32_t cap = in_len + in_len / 8 + 1024;
    const uint32_t maxb = lz_blocks(in_len);
    const size_t o_model = hc.take(model_bytes);
    m.in_off = hc.take(in_len, 64);
    m.out_off = hc.take(cap, 64);
    const size_t o_tok = hc.take(lz_scratch(1, maxb, 0).bytes, 64);
    m.in_len = in_len;
    m.out_cap = cap;
    memcpy(&m.rs, state_in, sizeof(m.rs));
    rc = hc.begin();
    if (rc) return rc;
    uint8_t *base = hc.at(0), *d_model = hc.at(o_model), *d_out = hc.at(m.out_off);
    Meta *dm = hc.dm;
    HIP_TRY(hc.put_meta());
    if (state_in->flags & 1u) HIP_TRY(mz_h2d(d_model, model, model_bytes));
    if (in_len) HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
    hipStream_t s = MZ_HOST_STREAM;
    LzmaEncResumeArgs r{};
    rc = lz_parse_one_stream(hc.c, s, r.a, base, dm, maxb, skip_blocks, preset, (uint32_t *)hc.at(o_tok));
    if (rc) return rc;
    r.skip_blocks = skip_blocks;
    r.rs = &dm->rs;
    r.st = last ? nullptr : &dm->st;
    r.model = (uint16_t *)d_model;
    hipLaunchKernelGGL(k_lzma_rc_encode_resume, dim3(1), dim3(64), 0, s, r);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail("k_lzma_rc_encode_resume", le);
    HIP_TRY(hc.wait_fetch_meta());
    if (m.status == 0 && m.out_len > out_cap) m.status = MZHIP_STATUS_OUT_FULL;
    if (m.status == 0 && m.out_len) HIP_TRY(mz_d2h(out, d_out, m.out_len));
    if (m.status == 0 && !last) {
        memcpy(state_out, &m.st, sizeof(m.st));
        HIP_TRY(mz_d2h(model, d_model, model_bytes));
    }
    give(out_len, m.out_len);
    return m.status;
}

// One .xz stream (single block, CRC32 check) from a host buffer: the block is parsed as one stream and cut into 64 KiB
// LZMA2 chunks that reset state and properties but keep the dictionary (xz_encode_impl below), so the range coding of all
// chunks is one launch of independent waves while their matches reach back over the whole block; framing bytes (a few per
// chunk) are laid out here, the CRC-32s come from the device as well.
int32_t mzhip_xz_encode_host(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_cap, uint32_t *out_len,
                             uint32_t *crc) {
    return mzhip_xz_encode_host_preset(in, in_len, 1, out, out_cap, out_len, crc);
}

// part = 0: a whole .xz stream (header, one block, index, footer).  part = 1: [the stream header when `first`] + ONE block;
// *unpadded receives the block's unpadded size for the index (mzhip_xz_encode_finish_host writes it)
static int32_t xz_encode_impl(const uint8_t *in, uint32_t in_len, int32_t preset, int part, int first, uint8_t *out, uint32_t out_cap,
                              uint32_t *out_len, uint32_t *crc, uint64_t *unpadded) {
    /* One .xz block = ONE parsed stream (round 4): the block's bytes go through the chain pass and the block parse as a
     * method-14 stream does -- a chunk's matches reach back over the chunks before it, 8 MiB at most -- and every 64 KiB
     * block of the parse becomes one LZMA2 chunk, range-coded by a wave of its own with a fresh coder and model (the first
     * chunk resets the dictionary, the others keep it: control 0xE0 / 0xC0).  Round 3's chunks were 48 KiB streams of
     * their own that reset the dictionary too: the writer then had a 48 KiB dictionary where liblzma's preset has 8 MiB. */
    const uint32_t piece = MZ_DEF_BLOCK;
    const uint32_t np = (in_len + piece - 1) / piece;
    const uint32_t pcap = piece + piece / 8 + 1024;
    struct Meta {
        uint64_t in_off, out_off;
        uint32_t in_len, out_cap, out_len, crc;
        int32_t status;
        uint32_t crc_init;
    };
    HostCall<Meta> hc;
    Meta &m = hc.m;
    const size_t o_chunk = hc.take((size_t)np * 2 * sizeof(uint32_t), 64); /* chunk_len[np], chunk_status[np] */
    m.in_off = hc.take(in_len, 64);
    m.out_off = hc.take((size_t)np * pcap, 64);
    const size_t o_tok = hc.take(lz_scratch(1, np, 0).bytes, 64);
    m.in_len = in_len;
    m.out_cap = pcap;
    int32_t rc = hc.begin();
    if (rc) return rc;
    DeviceCtx *c = hc.c;
    uint8_t *base = hc.at(0), *d_out = hc.at(m.out_off);
    std::vector<uint32_t> h_len(np ? np : 1, 0);
    std::vector<int32_t> h_status(np ? np : 1, 0);
    uint32_t total_crc = 0;
    if (np) {
        HIP_TRY(hc.put_meta());
        HIP_TRY(mz_h2d(hc.at(m.in_off), in, in_len));
        Meta *dm = hc.dm;
        hipStream_t s = MZ_HOST_STREAM;
        LzmaEncChunksArgs r{};
        rc = lz_parse_one_stream(c, s, r.a, base, dm, np, 0, preset, (uint32_t *)hc.at(o_tok));
        if (rc) return rc;
        r.nchunks = np;
        r.chunk_cap = pcap;
        r.chunk_len = (uint32_t *)hc.at(o_chunk);
        r.chunk_status = (int32_t *)(r.chunk_len + np);
        hipLaunchKernelGGL(k_lzma2_chunks_encode, dim3(resident_grid(np, (uint32_t)c->cu_count * 9u)), dim3(64), 0, s, r); /* 17 KiB LDS per single-wave workgroup */
        {
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) return fail("k_lzma2_chunks_encode", le);
        }
        /* the block's check: CRC-32 of its uncompressed bytes, where they lie */
        rc = mzhip_crc32_batch(base, &dm->in_off, &dm->in_len, 1, &dm->crc_init, &dm->crc, s);
        if (rc) return rc;
        HIP_TRY(hc.wait_fetch_meta());
        HIP_TRY(mz_d2h(h_len.data(), r.chunk_len, (size_t)np * sizeof(uint32_t)));
        HIP_TRY(mz_d2h(h_status.data(), r.chunk_status, (size_t)np * sizeof(int32_t)));
        total_crc = m.crc;
    }
    // ---- container (The .xz File Format 1.0.4): stream header, one block, index, footer
    uint32_t pos = 0;
    auto put = [&](const void *p, uint32_t n) -> bool {
        if (n > out_cap - pos) return false;
        memcpy(out + pos, p, n);
        pos += n;
        return true;
    };
    uint8_t hdr[12] = {0xFD, '7', 'z', 'X', 'Z', 0x00, 0x00, 0x01 /* check: CRC32 */, 0, 0, 0, 0};
    put_le32(hdr + 8, mzhip_crc32_host(0, hdr + 6, 2));
    uint8_t bh[12] = {0x02 /* (2 + 1) * 4 bytes */, 0x00 /* one filter, no sizes */, 0x21 /* LZMA2 */, 0x01,
                      (uint8_t)(np > 1u ? 0x16 /* 8 MiB: the reach of the parse's links */ : 0x08 /* 64 KiB */), 0, 0, 0, 0, 0, 0, 0};
    put_le32(bh + 8, mzhip_crc32_host(0, bh, 8));
    if ((!part || first) && !put(hdr, 12)) return MZHIP_STATUS_OUT_FULL;
    if (!put(bh, 12)) return MZHIP_STATUS_OUT_FULL;
    const uint32_t data_start = pos;
    int32_t loop_rc = 0; /* (copies into out[] may be in flight: every way out of the loop goes through the wait below) */
    for (uint32_t i = 0; i < np && !loop_rc; i++) {
        if (h_status[i] != 0 && h_status[i] != MZHIP_STATUS_OUT_FULL) { loop_rc = h_status[i]; break; }
        const uint32_t us = (in_len - i * piece < piece) ? in_len - i * piece : piece, cs = h_len[i];
        if (h_status[i] != 0 || cs >= us || cs > 65536u) {
            /* stored chunk: control 0x01 (dictionary reset) for the block's first chunk, 0x02 behind it -- the chunks that
             * follow look back into these bytes --, size - 1 big endian, the bytes */
            uint8_t ch[3] = {(uint8_t)(i == 0 ? 0x01 : 0x02), (uint8_t)((us - 1) >> 8), (uint8_t)(us - 1)};
            if (!put(ch, 3) || !put(in + (size_t)i * piece, us)) loop_rc = MZHIP_STATUS_OUT_FULL;
        } else { /* LZMA chunk: new properties and a fresh state; the first one resets the dictionary as well (0xE0), the
                    others keep it (0xC0) | size bits, sizes - 1, props */
            uint8_t ch[6] = {(uint8_t)((i == 0 ? 0xE0 : 0xC0) | ((us - 1) >> 16)), (uint8_t)((us - 1) >> 8), (uint8_t)(us - 1),
                             (uint8_t)((cs - 1) >> 8), (uint8_t)(cs - 1), MZ_LZE_PROPS};
            if (!put(ch, 6) || cs > out_cap - pos) { loop_rc = MZHIP_STATUS_OUT_FULL; break; }
            /* (the chunk lengths are on the host already: every copy is issued, one wait behind the loop -- an 8 MiB block was
             * 128 copy-and-wait round trips, ADVICE r4) */
            {
                const hipError_t ce = hipMemcpyAsync(out + pos, d_out + (size_t)i * pcap, cs, hipMemcpyDeviceToHost, MZ_HOST_STREAM);
                if (ce != hipSuccess) { loop_rc = fail("xz chunk copy", ce); break; }
            }
            pos += cs;
        }
    }
    HIP_TRY(hipStreamSynchronize(MZ_HOST_STREAM));
    if (loop_rc) return loop_rc;
    const uint8_t zero4[4] = {0, 0, 0, 0};
    if (!put(zero4, 1)) return MZHIP_STATUS_OUT_FULL; /* end of the LZMA2 data */
    const uint32_t csize_blk = pos - data_start;
    if (!put(zero4, (4u - (csize_blk & 3u)) & 3u)) return MZHIP_STATUS_OUT_FULL;
    uint8_t chk[4];
    put_le32(chk, total_crc);
    if (!put(chk, 4)) return MZHIP_STATUS_OUT_FULL;
    if (unpadded) *unpadded = 12ull + csize_blk + 4ull;
    if (!part) { /* a whole stream: the index over this one block and the footer */
        const uint64_t unp = 12ull + csize_blk + 4ull, unc = in_len;
        uint32_t tail = 0;
        rc = mzhip_xz_encode_finish_host(&unp, &unc, 1, out + pos, out_cap - pos, &tail);
        if (rc) return rc;
        pos += tail;
    }
    give(out_len, pos);
    give(crc, total_crc);
    return 0;
}

int32_t mzhip_xz_encode_host_preset(const uint8_t *in, uint32_t in_len, int32_t preset, uint8_t *out, uint32_t out_cap,
                                    uint32_t *out_len, uint32_t *crc) {
    return xz_encode_impl(in, in_len, preset, 0, 1, out, out_cap, out_len, crc, nullptr);
}

// A .xz stream written block by block in bounded memory (include/mzhip.h): one block per call ...
int32_t mzhip_xz_encode_block_host(const uint8_t *in, uint32_t in_len, int32_t preset, int32_t first, uint8_t *out, uint32_t out_cap,
                                   uint32_t *out_len, uint32_t *crc, uint64_t *unpadded_size) {
    if (!in_len || !unpadded_size) return -102; /* MZ_PARAM_ERROR: a block holds at least one byte */
    return xz_encode_impl(in, in_len, preset, 1, first, out, out_cap, out_len, crc, unpadded_size);
}

// One stream segment: split into pieces of def_stream_piece() bytes (one wave each, the 32 KiB in front as history); every piece but the
// last ends with an empty stored block so the pieces concatenate on byte boundaries; the last piece is final iff `final`.
static int32_t deflate_segment_host(const uint8_t *in, uint32_t in_len, uint32_t final, int32_t level, int32_t window_log2,
                                 uint8_t *out, uint32_t out_cap, uint32_t *out_len, uint32_t *crc, uint32_t *adler) {
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    const uint32_t piece = def_stream_piece(in_len, level);
    const uint32_t np = in_len ? (in_len + piece - 1) / piece : 1u;
    const uint32_t pcap = piece + piece / 8 + 64; /* fixed-Huffman worst case is 9/8 of the input */
    const size_t meta = (size_t)np * (8 + 8 + 4 + 4 + 4 + 4 + 4 + 4 + 4 + 1);
    const size_t meta_pad = (meta + 63) & ~(size_t)63;
    const size_t in_pad = ((size_t)in_len + 63) & ~(size_t)63;
    Staging sc;
    rc = sc.get(c, meta_pad + in_pad + (size_t)np * pcap);
    if (rc) return rc;
    uint8_t *base = (uint8_t *)sc.p;
    uint8_t *hm = (uint8_t *)calloc(1, meta_pad);
    if (!hm) return -4;
    uint64_t *h_in_off = (uint64_t *)hm, *h_out_off = h_in_off + np;
    uint32_t *h_in_len = (uint32_t *)(h_out_off + np), *h_out_cap = h_in_len + np, *h_out_len = h_out_cap + np,
             *h_crc = h_out_len + np;
    int32_t *h_status = (int32_t *)(h_crc + np);
    uint32_t *h_adler = (uint32_t *)(h_status + np);
    uint32_t *h_warm = h_adler + np;
    uint8_t *h_final = (uint8_t *)(h_warm + np);
    for (uint32_t i = 0; i < np; i++) {
        h_in_off[i] = meta_pad + (uint64_t)i * piece;
        h_warm[i] = def_stream_warm((uint64_t)i * piece);
        const uint32_t left = in_len - (in_len ? i * piece : 0);
        h_in_len[i] = left < piece ? left : piece;
        h_out_off[i] = meta_pad + in_pad + (uint64_t)i * pcap;
        h_out_cap[i] = pcap;
        h_final[i] = (uint8_t)((i + 1 == np && final) ? 1 : 0);
    }
    hipError_t he = mz_h2d(base, hm, meta);
    if (he == hipSuccess && in_len) he = mz_h2d(base + meta_pad, in, in_len);
    if (he != hipSuccess) {
        free(hm);
        return fail("hipMemcpy (deflate input)", he);
    }
    uint64_t *d_in_off = (uint64_t *)base, *d_out_off = d_in_off + np;
    uint32_t *d_in_len = (uint32_t *)(d_out_off + np), *d_out_cap = d_in_len + np, *d_out_len = d_out_cap + np,
             *d_crc = d_out_len + np;
    int32_t *d_status = (int32_t *)(d_crc + np);
    uint32_t *d_adler = (uint32_t *)(d_status + np);
    uint32_t *d_warm = d_adler + np;
    uint8_t *d_final = (uint8_t *)(d_warm + np);
    rc = deflate_batch_launch(base, d_in_off, d_in_len, d_warm, base, d_out_off, d_out_cap, d_final, np, level, window_log2, d_out_len,
                              d_crc, d_status, MZ_HOST_STREAM);
    if (rc == 0 && hipStreamSynchronize(MZ_HOST_STREAM) != hipSuccess) rc = -104;
    /* zlib wrapper: Adler-32 of the same pieces, one wave each, combined below from the checksums alone */
    if (rc == 0 && adler) rc = mzhip_adler32_batch(base, d_in_off, d_in_len, np, d_adler, MZ_HOST_STREAM);
    if (rc == 0 && adler && hipStreamSynchronize(MZ_HOST_STREAM) != hipSuccess) rc = -104;
    if (rc == 0 && mz_d2h(hm, base, meta) != hipSuccess) rc = -104;
    uint32_t total = 0, k = 0, ad = 1;
    /* many pieces: the device moves them together into the room the input took (it is done with), and ONE copy fetches them --
     * when they fit there, which anything that compresses at all does; a copy per piece otherwise */
    bool packed = false;
    if (rc == 0 && np > 2u) {
        uint64_t sum = 0;
        bool ok = true;
        for (uint32_t i = 0; i < np; i++) {
            if (h_status[i] != 0 || h_out_len[i] > pcap) ok = false;
            sum += h_out_len[i];
        }
        if (ok && sum <= in_pad && sum <= out_cap) {
            std::vector<uint64_t> dst(np);
            uint64_t at = 0;
            for (uint32_t i = 0; i < np; i++) {
                dst[i] = at;
                at += h_out_len[i];
            }
            PiecePackArgs pa{};
            pa.src = base;
            pa.src_off = d_out_off;
            pa.len = d_out_len;
            pa.dst = base + meta_pad;
            pa.dst_off = d_in_off; /* (the pieces' input offsets are done with as well) */
            pa.n = np;
            if (mz_h2d(d_in_off, dst.data(), (size_t)np * 8) == hipSuccess) {
                hipLaunchKernelGGL(k_pack_pieces, dim3(resident_grid(np, 1024u)), dim3(256), 0, MZ_HOST_STREAM, pa);
                if (hipGetLastError() == hipSuccess && (sum == 0 || mz_d2h(out, base + meta_pad, (size_t)sum) == hipSuccess)) packed = true;
                else rc = -104;
            } else
                rc = -104;
        }
    }
    for (uint32_t i = 0; rc == 0 && i < np; i++) {
        if (h_status[i] != 0) rc = h_status[i];
        else if (h_out_len[i] > out_cap - total) rc = MZHIP_STATUS_OUT_FULL;
        else if (!packed && mz_d2h(out + total, base + h_out_off[i], h_out_len[i]) != hipSuccess) rc = -104;
        else {
            total += h_out_len[i];
            k = (i == 0) ? h_crc[0] : mzhip_crc32_combine_host(k, h_crc[i], h_in_len[i]); /* checksums only */
            if (adler) ad = mzhip_adler32_combine_host(ad, h_adler[i], h_in_len[i]);
        }
    }
    free(hm);
    if (out_len) *out_len = total;
    if (crc) *crc = k;
    if (adler) *adler = ad;
    return rc;
}

int32_t mzhip_deflate_host_a(const mzhip_deflate_host_args *ap) {
    if (!ap || ap->size < offsetof(mzhip_deflate_host_args, out) + sizeof(void *) || ap->size > 4096u || (ap->size & 3u)) return -102; /* MZ_PARAM_ERROR */
    mzhip_deflate_host_args a;
    memset(&a, 0, sizeof(a));
    memcpy(&a, ap, ap->size < sizeof(a) ? ap->size : sizeof(a));
    return deflate_segment_host(a.in, a.in_len, a.final, a.level, a.window_log2 ? a.window_log2 : 15, a.out, a.out_cap,
                                a.out_len, a.crc, a.adler);
}

__attribute__((visibility("hidden"))) uint32_t mzhip_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) {
    return mzhip_adler32_combine_host(ad1, ad2, len2);
}

} // extern "C"

namespace {
const mzhip_crc_tables *host_crc_tables() {
    static mzhip_crc_tables t;
    static std::once_flag once;
    std::call_once(once, [] { mzhip_crc_tables_init(&t); });
    return &t;
}
} // namespace

uint32_t mzh::crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return mzhip_crc32_combine_host(crc_a, crc_b, len_b); }

uint32_t mzh::crc32_fold_host(uint32_t value, const uint8_t *p, size_t n) {
    const mzhip_crc_tables *t = host_crc_tables();
    uint32_t r = ~value; /* register inverted on entry and exit, mz_crypt.c:81,90 */
    while (n && ((uintptr_t)p & 3u)) {
        r = t->byte_tab[(r ^ *p++) & 255u] ^ (r >> 8);
        n--;
    }
    for (; n >= 4; n -= 4, p += 4) {
        uint32_t d;
        memcpy(&d, p, 4);
        const uint32_t x = r ^ d; /* little-endian host */
        r = t->slice[3][x & 255u] ^ t->slice[2][(x >> 8) & 255u] ^ t->slice[1][(x >> 16) & 255u] ^ t->slice[0][x >> 24];
    }
    while (n--) r = t->byte_tab[(r ^ *p++) & 255u] ^ (r >> 8);
    return ~r;
}
