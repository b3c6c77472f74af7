// mzhip_prime.inc -- the READ-side prime cache of libmzhip.so and its decode pipeline (host code, no device code).
// Textually included by mzhip_prime.cpp (which supplies DeviceCtx / ctx_for_current, HIP_TRY / fail / g_err through mzhip_runtime.h,
// Scratch, lzma_family_batch, mzhip_crc32_combine_host and the batch launchers of include/mzhip.h) -- and, as TEST INFRASTRUCTURE, by
// tests/emul/mock_device.cpp, which supplies the same names over
// a synchronous stand-in for the HIP runtime and the host emulation of the device cores, so that the cache, the pipeline and
// shim_autoprime.c run behind the unmodified zip layer in a container without a GPU (also under the sanitizers).

// ---------------------------------------------------------------------------------------------------------
// "Prime" path (SURVEY 8b, Batching): decode every DEFLATE entry of an archive in ONE launch and keep the result
// in a host cache, so that the reference's untouched one-entry-at-a-time loop (mz_zip_entry_read ->
// mz_stream_zlib_read -> mz_crypt_crc32_update) is served at memcpy speed.  The codec stream recognises a primed
// entry by the position of its base stream (= the payload offset) plus the first payload bytes; whatever it
// returns is still CRC-checked by mz_zip.c:2116-2128 against the central directory.  CRCs are GPU-computed:
// per entry, and per 65 535-byte segment (the reader's buffer size, mz_zip_rw.c:55) for the chunked updates.

namespace {
// Page-locked host memory is expensive to make (the pages are faulted in and pinned: ~100 ms per GiB) and a process that
// primes one archive after another needs the same two blocks again and again (the file image, the decoded bytes), so
// freed blocks are kept -- sixteen at most, 4 GiB in all -- and handed out again when they are large enough.  (Four slots
// until round 6: an archive that is rolled over cycles through two sizes of block, a window's image (~60 MB) and its decoded
// bytes (~200 MB), several of each in flight with more than one reader; four slots filled up with the wrong size, and most
// windows paid a hipHostMalloc and a hipHostFree of 200 MB -- tens of milliseconds each, and a process whose resident set
// overshot by what the runtime had not unpinned yet: 4.9 - 7.2 GB from run to run on the 110 000-entry archive.)
struct PinnedPool {
    std::mutex mu;
    static constexpr int kSlots = 16;
    std::atomic<uint64_t> made{0}, peak{0}; // bytes this pool has pinned and not given back yet, and the most that ever was (reports)
    void account(int64_t d) {
        const uint64_t now = made.fetch_add((uint64_t)d, std::memory_order_relaxed) + (uint64_t)d;
        uint64_t pk = peak.load(std::memory_order_relaxed);
        while (d > 0 && now > pk && !peak.compare_exchange_weak(pk, now, std::memory_order_relaxed)) {
        }
    }
    struct Blk {
        void *p = nullptr;
        size_t cap = 0;
    } blk[kSlots];
    void *get(size_t need, size_t *cap) {
        {
            std::lock_guard<std::mutex> lk(mu);
            int best = -1;
            for (int i = 0; i < kSlots; i++)
                if (blk[i].p && blk[i].cap >= need && (best < 0 || blk[i].cap < blk[best].cap)) best = i;
            if (best >= 0 && blk[best].cap <= 2 * need + ((size_t)64 << 20)) {
                void *p = blk[best].p;
                *cap = blk[best].cap;
                blk[best] = Blk();
                return p;
            }
        }
        void *p = nullptr;
        /* (in steps of 32 MiB from 64 MiB on: the windows of a rolled archive differ by a few MB, and a freed block should fit the next one) */
        static const size_t big_step = [] {
            const char *e = getenv("MZHIP_POOL_STEP_MB"); /* (A/B) */
            const long v = e ? atol(e) : 0;
            return (size_t)(v > 0 ? v : 32) << 20;
        }();
        const size_t step = need >= ((size_t)64 << 20) ? big_step : (size_t)2 << 20;
        const size_t want = (need + step) & ~(step - 1);
        /* the pages are placed where the thread that pins them runs, and that should be next to the current device (the
         * copy engines read and write this block): a thread of the library's own binds itself there for the allocation.
         * (It used to be the caller's thread, re-bound for the length of the call: runtime helper threads spawned in that
         * window inherited the narrow mask, ADVICE r3.) */
        int dev = 0;
        hipError_t he = hipGetDevice(&dev);
        if (he == hipSuccess) {
            std::thread t([&] {
                (void)mzhip_bind_thread_near_device(dev, 0);
                he = hipSetDevice(dev);
                if (he == hipSuccess) he = hipHostMalloc(&p, want, hipHostMallocDefault);
            });
            t.join();
        }
        if (he != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        *cap = want;
        account((int64_t)want);
        return p;
    }
    void put(void *p, size_t cap) {
        if (!p) return;
        void *drop = p;
        size_t drop_cap = cap;
        {
            std::lock_guard<std::mutex> lk(mu);
            /* blocks of the size a window takes (below 512 MiB) are kept up to 768 MiB in all: what lies idle here is resident
             * beside the windows that are live, and a reader that rolls over an archive frees as many as it makes.  The blocks
             * of a whole image (an application that primes archive after archive) are kept up to 4 GiB, as ever. */
            const size_t small_class = (size_t)512 << 20;
            size_t total = cap, total_small = cap < small_class ? cap : 0;
            int empty = -1, smallest = -1;
            for (int i = 0; i < kSlots; i++) {
                if (!blk[i].p) {
                    if (empty < 0) empty = i;
                    continue;
                }
                total += blk[i].cap;
                if (blk[i].cap < small_class) total_small += blk[i].cap;
                if (smallest < 0 || blk[i].cap < blk[smallest].cap) smallest = i;
            }
            static const size_t small_idle = [] {
                const char *e = getenv("MZHIP_POOL_IDLE_MB"); /* (A/B) idle window-sized blocks kept, MiB */
                const long v = e ? atol(e) : 0;
                return (size_t)(v > 0 ? v : 768) << 20;
            }();
            static const int slots = [] {
                const char *e = getenv("MZHIP_POOL_SLOTS"); /* (A/B) */
                const int v = e ? atoi(e) : 0;
                return v > 0 && v < kSlots ? v : (int)kSlots;
            }();
            int used = 0;
            for (int i = 0; i < kSlots; i++) used += blk[i].p ? 1 : 0;
            if (used >= slots) empty = -1;
            if (total <= ((size_t)4 << 30) && (cap >= small_class || total_small <= small_idle)) {
                if (empty >= 0) {
                    blk[empty].p = p;
                    blk[empty].cap = cap;
                    drop = nullptr;
                } else if (blk[smallest].cap < cap) {
                    drop = blk[smallest].p;
                    drop_cap = blk[smallest].cap;
                    blk[smallest].p = p;
                    blk[smallest].cap = cap;
                }
            }
        }
        if (drop) {
            (void)hipHostFree(drop);
            account(-(int64_t)drop_cap);
        }
    }
};
// (on the heap and never destroyed: a process that exits with generations still cached -- an application that never clears, the
// windows of a rolled archive -- must not hand page-locked blocks back to a HIP runtime that is being torn down: SIGSEGV at exit)
PinnedPool &g_pinned = *new PinnedPool();
} // namespace
extern "C" {
void *mzhip_window_alloc(size_t bytes, size_t *cap) {
    size_t c = 0;
    void *p = g_pinned.get(bytes, &c);
    if (cap) *cap = c;
    return p;
}
void mzhip_window_free(void *p, size_t cap) { g_pinned.put(p, cap); }
/* (reports, tests) page-locked bytes the pool holds or has handed out right now / at most so far */
__attribute__((visibility("default"))) void mzhip_pinned_stats(uint64_t *now, uint64_t *peak) {
    if (now) *now = g_pinned.made.load(std::memory_order_relaxed);
    if (peak) *peak = g_pinned.peak.load(std::memory_order_relaxed);
}
}
namespace {
double prime_now() {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
bool prime_trace() {
    static const bool on = getenv("MZHIP_PRIME_TRACE") != nullptr;
    return on;
}
struct PrimedEntry {
    int64_t payload_off, csize, usize, out_off;
    uint32_t crc;
    int32_t status;
    int64_t seg0; // index of this entry's first segment CRC
    int32_t method;
    int32_t head_len;
    uint8_t head[256]; // the first payload bytes: a stream must present the same ones to be served
    // the entry's Hash extra field (0x1a51, mz_zip_rw.c:1398-1408), when it names SHA-1 or SHA-256 -- the two the reader
    // verifies (mz_zip_rw.c:414-419): the digest of the decoded bytes is computed on the device in the pass that decodes
    // them and compared with the field's; an entry whose digest differs is not served from the cache
    uint16_t hash_alg, hash_size; // 0: no such field
    uint8_t hash_want[32], hash_got[32];
};
// One primed archive.  Generations are reference-counted: an open stream that is being served from one pins it, so a
// later prime / clear (another archive, another thread, MZHIP_AUTOPRIME) never frees memory a stream still reads.
struct PrimeGen {
    std::vector<PrimedEntry> entries; // sorted by payload_off
    std::vector<int64_t> offs;        // ... and the payload offsets alone: what a look-up searches (8 bytes a probe instead of a 400-byte
                                      // entry's cache line; a generation whose range does not hold the offset is not searched at all --
                                      // the windows of a rolled archive are a dozen generations with disjoint ranges)
    std::vector<uint32_t> seg_crc;
    uint8_t *out = nullptr; // page-locked (hipHostMalloc, from g_pinned): the D2H copy of the decoded bytes runs at link speed
    uint64_t out_bytes = 0; // ... of which the entries take this many
    bool out_pinned = false;
    size_t out_cap = 0;
    uint64_t zip_len = 0, ident = 0; // archive identity: length + hash of its central directory and end records
    bool window = false; // one window of an archive that shim_autoprime.c rolls over (ident = the archive's identity mixed with the
                         // window's first byte): such generations come and go under that file's budget, see mzhip_prime_window_begin
    // STORE entries: no codec stream sees them (the reference's raw stream hands the bytes to mz_crypt_crc32_update,
    // mz_zip.c:2047-2049), so the CRC symbol recognises a chunk by content: the payloads are kept, cut into the reader's
    // 65 535-byte chunks with their device-computed CRCs, indexed by a fingerprint of each chunk
    struct StoreSeg {
        uint64_t off; // into store[]
        uint32_t len, crc;
    };
    std::vector<StoreSeg> store_segs;
    std::unordered_multimap<uint64_t, uint32_t> store_idx; // fingerprint -> segment
    uint8_t *store = nullptr;
    bool store_pinned = false;
    uint64_t store_entries = 0;
    // A generation is published BEFORE its entries are decoded (a reader thread that asks for an entry whose chunk of
    // the decode pipeline has not landed yet waits for exactly that chunk, not for the whole archive): state[i] says
    // whether entries[i] may be served.  Entries are immutable but for `crc`, which is written before state turns 1;
    // the STORE index is built last and looked at only once store_ready is set.
    std::unique_ptr<std::atomic<uint8_t>[]> state; // 0 pending, 1 servable, 2 not served (did not decode to its declared sizes)
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<bool> store_ready{false};
    ~PrimeGen() {
        if (out_pinned) g_pinned.put(out, out_cap);
        else free(out);
        if (store_pinned) (void)hipHostFree(store);
        else free(store);
    }
};
struct PrimeCache {
    std::vector<std::shared_ptr<PrimeGen>> gens; // newest first, at most kMaxGens
};
PrimeCache &g_prime = *new PrimeCache(); // (never destroyed, like the pool: see there)
// readers (one lookup per entry that is opened, from as many host threads as the application has) share the lock;
// publishing, replacing and clearing a generation take it exclusively
std::shared_mutex g_prime_mu;
std::atomic<uint64_t> g_prime_hits{0}, g_prime_misses{0};
std::atomic<uint64_t> g_prime_hash_checked{0}, g_prime_hash_bad{0}; // entries whose Hash field was verified on the device / differed
std::atomic<uint64_t> g_prime_wait_ns{0}, g_prime_wait_n{0}; // MZHIP_PRIME_TRACE: lookups that had to wait for their chunk
std::atomic<int> g_any_gens{0};   // generations present at all: the streams' "is there anything to look up" (mzhip_prime_any)
std::atomic<int> g_store_gens{0}; // generations that hold STORE chunks: the CRC symbol's fast "nothing to look up"
std::atomic<uint64_t> g_prime_clears{0}; // mzhip_prime_clear() calls: shim_autoprime.c notices that its windows are gone
constexpr uint32_t kSeg = 65535u;
constexpr size_t kMaxGens = 64; // (whole archives primed side by side + the windows of the ones that are rolled over)

uint64_t fnv1a64(const uint8_t *p, uint64_t n, uint64_t h = 0xCBF29CE484222325ull) {
    for (uint64_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}
// fingerprint of a chunk of at least 32 bytes: its length, first and last 16 bytes (a hint only: a hit is confirmed
// byte by byte)
uint64_t store_key(const uint8_t *p, uint32_t n) {
    uint64_t h = fnv1a64((const uint8_t *)&n, 4);
    h = fnv1a64(p, 16, h);
    return fnv1a64(p + n - 16, 16, h);
}
void count_store_gens_locked() {
    int k = 0;
    for (const auto &g : g_prime.gens) k += (g->store_ready.load() && !g->store_segs.empty()) ? 1 : 0;
    g_store_gens.store(k);
    g_any_gens.store((int)g_prime.gens.size());
}
} // namespace

extern "C" {

void mzhip_prime_clear(void) {
    (void)mzhip_prime_wait(); /* a prime that is still running reads the caller's image: it is finished, then dropped */
    std::unique_lock<std::shared_mutex> lk(g_prime_mu);
    g_prime = PrimeCache(); // generations pinned by open streams live until those streams let go
    g_prime_clears.fetch_add(1, std::memory_order_relaxed);
    g_prime_hits.store(0);
    g_prime_misses.store(0);
    g_store_gens.store(0);
    g_any_gens.store(0);
}

} // extern "C"

namespace {
// One slice of the primed entries, decoded on the CURRENT device of the calling thread, as a PIPELINE: the slice is
// cut into chunks of about kPrimeChunk decoded bytes, and chunk i's H2D copy (the byte range of the archive that holds
// its payloads), its launches (one per codec + the segment CRCs) and its D2H copies (results and every decoded byte)
// are queued on stream i % 3, so that H2D(i + 1), kernel(i) and D2H(i - 1) run at the same time and the PCIe link is
// busy in both directions while the kernels run (round 2: blocking copies and a device-wide synchronisation around one
// launch per codec -- 31 GB/s over the link, VERDICT r2 weak 6).  Only the stream that is about to be reused is waited
// for, never the device.  ents[lo..hi) are in archive order; results land in the shared per-entry arrays.
constexpr uint64_t kPrimeChunk = 48ull << 20;
// DEFLATE entries of this many compressed bytes and more leave the batch launch and are decoded by a wave per block
// (mzhip_inflate_large); MZHIP_PRIME_LARGE=0 keeps them in the batch (one wave per entry, as before round 4)
constexpr int64_t kPrimeLargeEntry = 4ll << 20;
static int mzhip_prime_large_on() {
    static const int on = [] {
        const char *e = getenv("MZHIP_PRIME_LARGE");
        return (e && e[0] == '0') ? 0 : 1;
    }();
    return on;
}
constexpr int kPrimeLanes = 3;
struct PrimeLane {
    hipStream_t s = nullptr;
    Scratch d_zip, d_out, d_meta;
    size_t zip_cap = 0, out_cap = 0, meta_cap = 0;
    uint8_t *h_meta = nullptr; // page-locked staging: launch arrays up, results down
    size_t h_cap = 0;
    // the chunk in flight on this lane
    bool busy = false;
    size_t lo = 0, hi = 0;
    uint32_t k = 0, ns = 0;
    int64_t seg0 = 0;
    std::vector<uint32_t> order;
    size_t res_off = 0; // where the result arrays start inside h_meta
    std::vector<size_t> hash_ent; // entries of the chunk whose digests were asked for, in launch order ...
    size_t hash_off = 0;          // ... and where their 32-byte digests land inside h_meta
    ~PrimeLane() {
        if (s) (void)hipStreamDestroy(s);
        if (h_meta) (void)hipHostFree(h_meta);
    }
};
struct PrimeLaneSet {
    PrimeLane lanes[kPrimeLanes];
};
std::mutex g_lane_mu;
// Parked lane sets, per device.  A set that has been made is NEVER destroyed: the scratch and work-queue caches of the runtime
// keep events that were recorded on a lane's stream (the leases of mzhip_slots.inc) and ask them later, and this HIP runtime
// looks at the stream an event was last recorded on -- after hipStreamDestroy that is freed memory, and the answer was
// "operation not permitted when stream is capturing" for some later launch of some other thread (found in round 6, when the
// windows of a rolled archive made two primes at once -- and with it a second, short-lived set -- the normal case).  As many
// sets as primes ever ran at once on the device exist, each idle one parked here.
std::vector<PrimeLaneSet *> *g_lane_sets[kMaxDevices]; // (never destroyed at exit either: the runtime may be gone before static destructors run)
int32_t prime_lane_reserve(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return 0;
    if (*p) HIP_TRY(hipFree(*p)); // (the lane's stream has been waited for: nothing uses the buffer)
    *p = nullptr;
    *cap = 0;
    const size_t want = (need + (need >> 2) + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
    HIP_TRY(hipMalloc(p, want));
    *cap = want;
    return 0;
}
// results of the chunk that ran on lane L: wait for its stream (only this one); the entries that decoded cleanly, to
// their declared sizes, become servable (everything else goes through the ordinary per-entry path and its exact error
// behaviour) and the readers that wait for them are woken
int32_t prime_lane_collect(PrimeLane &L, PrimeGen *gen) {
    if (!L.busy) return 0;
    HIP_TRY(hipStreamSynchronize(L.s));
    const uint32_t k = L.k;
    const uint32_t *h_len = (const uint32_t *)(L.h_meta + L.res_off), *h_used = h_len + k, *h_crc = h_used + k;
    const int32_t *h_st = (const int32_t *)(h_crc + k);
    const uint32_t *h_seg = (const uint32_t *)(h_st + k);
    if (L.ns) memcpy(gen->seg_crc.data() + L.seg0, h_seg, (size_t)L.ns * 4);
    for (uint32_t i = 0; i < k; i++) {
        const size_t g = L.lo + L.order[i];
        PrimedEntry &e = gen->entries[g];
        const bool good = h_st[i] == 0 && h_len[i] == (uint32_t)e.usize && h_used[i] == (uint32_t)e.csize;
        e.crc = h_crc[i];
        e.status = good ? 0 : (h_st[i] ? h_st[i] : -3);
        if (!e.hash_alg) gen->state[g].store(good ? 1 : 2, std::memory_order_release);
    }
    /* entries with a SHA-1 / SHA-256 Hash field: servable only if the digest of what was decoded is the field's (the
     * reference compares the field's digest_size bytes, mz_zip_rw.c:446-449) */
    for (size_t j = 0; j < L.hash_ent.size(); j++) {
        PrimedEntry &e = gen->entries[L.hash_ent[j]];
        memcpy(e.hash_got, L.h_meta + L.hash_off + 32 * j, 32);
        const uint32_t full = e.hash_alg == 20 ? 20u : 32u;
        const uint32_t cmp = e.hash_size < full ? e.hash_size : full;
        const bool same = e.status == 0 && e.hash_size <= 64 && memcmp(e.hash_got, e.hash_want, cmp) == 0;
        if (e.status == 0) {
            g_prime_hash_checked.fetch_add(1, std::memory_order_relaxed);
            if (!same) g_prime_hash_bad.fetch_add(1, std::memory_order_relaxed);
        }
        gen->state[L.hash_ent[j]].store(same ? 1 : 2, std::memory_order_release);
    }
    { std::lock_guard<std::mutex> lk(gen->mu); } /* (a waiter is either before its check or inside wait()) */
    gen->cv.notify_all();
    {
        static const bool each = getenv("MZHIP_PRIME_TRACE") && atoi(getenv("MZHIP_PRIME_TRACE")) >= 2;
        if (each) fprintf(stderr, "[mzhip prime] entries %zu..%zu servable at %.2f ms\n", L.lo, L.hi, prime_now() * 1e3);
    }
    L.busy = false;
    return 0;
}
// (zip[0] = byte `bias` of the archive: the whole image, or the window of it a rolling prime holds)
int32_t prime_slice(const uint8_t *zip, uint64_t bias, PrimeGen *gen, const std::vector<int64_t> &max_out_all, size_t lo, size_t hi) {
    std::vector<PrimedEntry> &ents = gen->entries;
    uint8_t *const h_out = gen->out;
    DeviceCtx *c = nullptr;
    int32_t rc = ctx_for_current(&c);
    if (rc) return rc;
    if (hi <= lo) return 0;
    /* streams, device buffers and page-locked staging of the three lanes are kept between calls (idle sets are parked per
     * device; a prime that finds none makes one, and it is parked afterwards like the others): hipMalloc / hipFree /
     * hipHostMalloc of ~200 MB per call cost more than the pipeline itself on a 1 GiB archive (44 ms -> see profiles/r3) */
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    PrimeLaneSet *set = nullptr;
    if (dev < 0 || dev >= kMaxDevices) return -102;
    {
        std::lock_guard<std::mutex> lk(g_lane_mu);
        if (!g_lane_sets[dev]) g_lane_sets[dev] = new std::vector<PrimeLaneSet *>();
        if (!g_lane_sets[dev]->empty()) {
            set = g_lane_sets[dev]->back();
            g_lane_sets[dev]->pop_back();
        }
    }
    if (!set) {
        set = new PrimeLaneSet();
        for (auto &L : set->lanes)
            if (hipStreamCreateWithFlags(&L.s, hipStreamNonBlocking) != hipSuccess) L.s = nullptr;
    }
    struct Park { /* back to the shelf on EVERY way out.  After a failure in the middle its lanes may still have work queued:
                     they are waited for first (the buffers the work uses belong to the set and stay) */
        PrimeLaneSet *set;
        int dev;
        bool ok = false;
        ~Park() {
            for (auto &L : set->lanes) {
                if ((L.busy || !ok) && L.s) (void)hipStreamSynchronize(L.s);
                L.busy = false;
            }
            std::lock_guard<std::mutex> lk(g_lane_mu);
            g_lane_sets[dev]->push_back(set);
        }
    } park{set, dev};
    for (auto &L : set->lanes)
        if (!L.s) return fail("hipStreamCreateWithFlags", (hipError_t)2 /* hipErrorOutOfMemory */);
    PrimeLane *lanes = set->lanes;
    int turn = 0;
    for (size_t c0 = lo; c0 < hi;) {
        /* the next chunk: entries [c0, c1), about kPrimeChunk decoded bytes (one entry at least) */
        size_t c1 = c0;
        uint64_t acc = 0;
        while (c1 < hi && (c1 == c0 || acc + (uint64_t)ents[c1].usize + (uint64_t)ents[c1].csize <= kPrimeChunk)) {
            acc += (uint64_t)ents[c1].usize + (uint64_t)ents[c1].csize;
            c1++;
        }
        PrimeLane &L = lanes[turn];
        turn = (turn + 1) % kPrimeLanes;
        rc = prime_lane_collect(L, gen); /* the chunk this lane ran three chunks ago */
        if (rc) return rc;
        const uint32_t k = (uint32_t)(c1 - c0);
        uint64_t zlo = UINT64_MAX, zhi = 0;
        for (size_t i = c0; i < c1; i++) {
            zlo = std::min(zlo, (uint64_t)ents[i].payload_off);
            zhi = std::max(zhi, (uint64_t)(ents[i].payload_off + ents[i].csize));
        }
        const int64_t out_base = ents[c0].out_off;
        const uint64_t out_bytes = (uint64_t)(ents[c1 - 1].out_off - out_base) + (((uint64_t)ents[c1 - 1].usize + 15) & ~15ull);
        uint32_t ns = 0;
        for (size_t i = c0; i < c1; i++) ns += (uint32_t)((ents[i].usize + kSeg - 1) / kSeg);
        /* launch arrays (grouped by method: one batch launch per codec) and result arrays, one page-locked block:
         *   up:   in_off[k] out_off[k] seg_off[ns] max_out[k] (8 bytes each)  in_len[k] out_cap[k] seg_len[ns] (4 bytes each)
         *   down: out_len[k] in_used[k] crc[k] status[k] seg_crc[ns] */
        const size_t up = (size_t)k * 24 + (size_t)ns * 8 + (size_t)k * 8 + (size_t)ns * 4;
        const size_t down = (size_t)k * 16 + (size_t)ns * 4;
        const size_t up_al = (up + 255) & ~(size_t)255;
        /* ... and for the entries with a SHA-1 / SHA-256 Hash field: off[kh] (8 bytes), len[kh] (4) up, digest[kh] (32) down */
        L.hash_ent.clear();
        for (int pass = 0; pass < 2; pass++)
            for (size_t i = c0; i < c1; i++)
                if (ents[i].hash_alg == (pass == 0 ? 20 : 23)) L.hash_ent.push_back(i); /* SHA-1 first, then SHA-256: one launch each */
        const size_t kh = L.hash_ent.size();
        const size_t down_al = (down + 255) & ~(size_t)255;
        const size_t hup = kh * 12, hup_al = (hup + 255) & ~(size_t)255, hdown = kh * 32;
        const size_t meta_all = up_al + down_al + hup_al + hdown;
        if (meta_all > L.h_cap) {
            if (L.h_meta) HIP_TRY(hipHostFree(L.h_meta));
            L.h_meta = nullptr;
            L.h_cap = 0;
            const size_t want = (meta_all * 2 + 4095) & ~(size_t)4095;
            HIP_TRY(hipHostMalloc((void **)&L.h_meta, want, hipHostMallocDefault));
            L.h_cap = want;
        }
        rc = prime_lane_reserve(&L.d_zip.p, &L.zip_cap, (size_t)(zhi - zlo) + 16);
        if (!rc) rc = prime_lane_reserve(&L.d_out.p, &L.out_cap, (size_t)out_bytes + 16);
        if (!rc) rc = prime_lane_reserve(&L.d_meta.p, &L.meta_cap, meta_all + 256);
        if (rc) return rc;
        L.order.resize(k);
        for (uint32_t i = 0; i < k; i++) L.order[i] = i;
        std::stable_sort(L.order.begin(), L.order.end(), [&](uint32_t a, uint32_t b) { return ents[c0 + a].method < ents[c0 + b].method; });
        uint64_t *h_in_off = (uint64_t *)L.h_meta, *h_out_off = h_in_off + k, *h_seg_off = h_out_off + k;
        int64_t *h_max_out = (int64_t *)(h_seg_off + ns);
        uint32_t *h_in_len = (uint32_t *)(h_max_out + k), *h_out_cap = h_in_len + k, *h_seg_len = h_out_cap + k;
        for (uint32_t i = 0; i < k; i++) {
            const PrimedEntry &e = ents[c0 + L.order[i]];
            h_in_off[i] = (uint64_t)e.payload_off - zlo;
            h_in_len[i] = (uint32_t)e.csize;
            h_out_off[i] = (uint64_t)(e.out_off - out_base);
            h_out_cap[i] = (uint32_t)e.usize;
            h_max_out[i] = max_out_all[c0 + L.order[i]];
            /* a large DEFLATE entry is not for one wave (0.1 - 0.2 GB/s): the batch launch sees it empty, and it is decoded
             * right behind that launch by a wave per block (mzhip_inflate_large) */
            if (e.method == 8 && e.csize >= kPrimeLargeEntry && mzhip_prime_large_on()) h_in_len[i] = 0;
        }
        { // segments for the chunked CRC updates, in archive order (seg0 was assigned by the caller)
            uint32_t j = 0;
            for (size_t i = c0; i < c1; i++)
                for (int64_t o = 0; o < ents[i].usize; o += kSeg) {
                    h_seg_off[j] = (uint64_t)(ents[i].out_off - out_base) + (uint64_t)o;
                    h_seg_len[j] = (uint32_t)(ents[i].usize - o < kSeg ? ents[i].usize - o : kSeg);
                    j++;
                }
        }
        uint8_t *m = (uint8_t *)L.d_meta.p;
        uint64_t *d_in_off = (uint64_t *)m, *d_out_off = d_in_off + k, *d_seg_off = d_out_off + k;
        int64_t *d_max_out = (int64_t *)(d_seg_off + ns);
        uint32_t *d_in_len = (uint32_t *)(d_max_out + k), *d_out_cap = d_in_len + k, *d_seg_len = d_out_cap + k;
        uint32_t *d_out_len = (uint32_t *)(m + up_al), *d_in_used = d_out_len + k, *d_crc = d_in_used + k;
        int32_t *d_status = (int32_t *)(d_crc + k);
        uint32_t *d_seg_crc = (uint32_t *)(d_status + k);
        HIP_TRY(hipMemcpyAsync(L.d_zip.p, zip + (zlo - bias), zhi - zlo, hipMemcpyHostToDevice, L.s));
        HIP_TRY(hipMemcpyAsync(m, L.h_meta, up, hipMemcpyHostToDevice, L.s));
        for (uint32_t g0 = 0; g0 < k;) {
            uint32_t g1 = g0;
            const int32_t method = ents[c0 + L.order[g0]].method;
            while (g1 < k && ents[c0 + L.order[g1]].method == method) g1++;
            const uint32_t gn = g1 - g0;
            if (method == 8)
                rc = mzhip_inflate_batch(L.d_zip.p, d_in_off + g0, d_in_len + g0, L.d_out.p, d_out_off + g0, d_out_cap + g0, gn,
                                         d_out_len + g0, d_in_used + g0, d_crc + g0, d_status + g0, L.s);
            else
                rc = lzma_family_batch(method == 95, L.d_zip.p, d_in_off + g0, d_in_len + g0, L.d_out.p, d_out_off + g0,
                                       d_out_cap + g0, d_max_out + g0, gn, d_out_len + g0, d_in_used + g0, d_crc + g0,
                                       d_status + g0, L.s);
            if (rc) return rc;
            g0 = g1;
        }
        for (uint32_t i = 0; i < k; i++) {
            const PrimedEntry &e = ents[c0 + L.order[i]];
            if (!(e.method == 8 && e.csize >= kPrimeLargeEntry && mzhip_prime_large_on())) continue;
            uint32_t r4[4] = {0, 0, 0, 0};
            int32_t st = 0;
            rc = mzhip_inflate_large((const uint8_t *)L.d_zip.p + h_in_off[i], (uint32_t)e.csize, (uint8_t *)L.d_out.p + h_out_off[i],
                                     (uint32_t)e.usize, &r4[0], &r4[1], &r4[2], &st, L.s);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(d_out_len + i, &r4[0], 4, hipMemcpyHostToDevice, L.s));
            HIP_TRY(hipMemcpyAsync(d_in_used + i, &r4[1], 4, hipMemcpyHostToDevice, L.s));
            HIP_TRY(hipMemcpyAsync(d_crc + i, &r4[2], 4, hipMemcpyHostToDevice, L.s));
            HIP_TRY(hipMemcpyAsync(d_status + i, &st, 4, hipMemcpyHostToDevice, L.s));
            HIP_TRY(hipStreamSynchronize(L.s)); /* (the four words live on this stack frame) */
        }
        if (ns) {
            rc = mzhip_crc32_batch(L.d_out.p, d_seg_off, d_seg_len, ns, nullptr, d_seg_crc, L.s);
            if (rc) return rc;
        }
        if (kh) {
            /* the digests of the decoded bytes, while they are in HBM (what mz_zip_reader_entry_read hashes 65 535 bytes at a
             * time on the host, mz_zip_rw.c:465-466): one lane per entry, one launch per algorithm */
            uint64_t *h_hoff = (uint64_t *)(L.h_meta + up_al + down_al);
            uint32_t *h_hlen = (uint32_t *)(h_hoff + kh);
            size_t n1 = 0;
            for (size_t j = 0; j < kh; j++) {
                const PrimedEntry &e = ents[L.hash_ent[j]];
                h_hoff[j] = (uint64_t)(e.out_off - out_base);
                h_hlen[j] = (uint32_t)e.usize;
                n1 += e.hash_alg == 20 ? 1 : 0;
            }
            uint64_t *d_hoff = (uint64_t *)(m + up_al + down_al);
            uint32_t *d_hlen = (uint32_t *)(d_hoff + kh);
            uint8_t *d_dig = m + up_al + down_al + hup_al;
            HIP_TRY(hipMemcpyAsync(d_hoff, h_hoff, hup, hipMemcpyHostToDevice, L.s));
            if (n1) rc = mzhip_sha_batch(L.d_out.p, d_hoff, d_hlen, (uint32_t)n1, 20, d_dig, L.s);
            if (!rc && kh > n1) rc = mzhip_sha_batch(L.d_out.p, d_hoff + n1, d_hlen + n1, (uint32_t)(kh - n1), 23, d_dig + 32 * n1, L.s);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(L.h_meta + up_al + down_al + hup_al, d_dig, hdown, hipMemcpyDeviceToHost, L.s));
            L.hash_off = up_al + down_al + hup_al;
        }
        HIP_TRY(hipMemcpyAsync(L.h_meta + up_al, m + up_al, down, hipMemcpyDeviceToHost, L.s));
        HIP_TRY(hipMemcpyAsync(h_out + out_base, L.d_out.p, out_bytes, hipMemcpyDeviceToHost, L.s));
        L.busy = true;
        L.lo = c0;
        L.hi = c1;
        L.k = k;
        L.ns = ns;
        L.seg0 = ents[c0].seg0;
        L.res_off = up_al;
        c0 = c1;
    }
    for (int i = 0; i < kPrimeLanes; i++) { /* in the order they were started */
        rc = prime_lane_collect(lanes[(turn + i) % kPrimeLanes], gen);
        if (rc) return rc;
    }
    park.ok = true;
    return 0;
}
// STORE entries of a primed archive: their payloads are copied into the generation, cut into the reader's chunks
// (kSeg bytes from the start of each entry), and every chunk's CRC-32 is computed on the current device, one launch
// per <= 1 GiB of payload.
int32_t prime_store(const uint8_t *zip, uint64_t bias, const std::vector<std::pair<int64_t, int64_t>> &stores, PrimeGen *gen) {
    uint64_t total = 0;
    for (const auto &e : stores) total += ((uint64_t)e.second + 15) & ~15ull;
    if (!total) return 0;
    gen->store_pinned = hipHostMalloc((void **)&gen->store, total + 16, hipHostMallocDefault) == hipSuccess;
    if (!gen->store_pinned) {
        (void)hipGetLastError();
        gen->store = (uint8_t *)malloc(total + 16);
    }
    if (!gen->store) return -4;
    uint64_t pos = 0;
    for (const auto &e : stores) {
        memcpy(gen->store + pos, zip + ((uint64_t)e.first - bias), (size_t)e.second);
        for (int64_t o = 0; o < e.second; o += kSeg)
            gen->store_segs.push_back({pos + (uint64_t)o, (uint32_t)(e.second - o < kSeg ? e.second - o : kSeg), 0u});
        pos += ((uint64_t)e.second + 15) & ~15ull;
    }
    const size_t ns = gen->store_segs.size();
    constexpr uint64_t kGroup = 1ull << 30;
    for (size_t s0 = 0; s0 < ns;) {
        size_t s1 = s0;
        const uint64_t base = gen->store_segs[s0].off;
        while (s1 < ns && gen->store_segs[s1].off + gen->store_segs[s1].len - base <= kGroup) s1++;
        const uint32_t gn = (uint32_t)(s1 - s0);
        const uint64_t bytes = gen->store_segs[s1 - 1].off + gen->store_segs[s1 - 1].len - base;
        std::vector<uint64_t> off(gn);
        std::vector<uint32_t> len(gn), crc(gn);
        for (uint32_t i = 0; i < gn; i++) {
            off[i] = gen->store_segs[s0 + i].off - base;
            len[i] = gen->store_segs[s0 + i].len;
        }
        Scratch d_buf, d_meta;
        HIP_TRY(hipMalloc(&d_buf.p, bytes + 16));
        HIP_TRY(hipMalloc(&d_meta.p, (size_t)gn * 16 + 64));
        uint64_t *d_off = (uint64_t *)d_meta.p;
        uint32_t *d_len = (uint32_t *)(d_off + gn), *d_crc = d_len + gn;
        HIP_TRY(hipMemcpy(d_buf.p, gen->store + base, bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_off, off.data(), (size_t)gn * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_len, len.data(), (size_t)gn * 4, hipMemcpyHostToDevice));
        const int32_t rc = mzhip_crc32_batch(d_buf.p, d_off, d_len, gn, nullptr, d_crc, nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr)); /* the launches above are on the null stream */
        HIP_TRY(hipMemcpy(crc.data(), d_crc, (size_t)gn * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < gn; i++) gen->store_segs[s0 + i].crc = crc[i];
        s0 = s1;
    }
    for (size_t i = 0; i < ns; i++) {
        const PrimeGen::StoreSeg &sg = gen->store_segs[i];
        if (sg.len >= 32u) gen->store_idx.emplace(store_key(gen->store + sg.off, sg.len), (uint32_t)i);
    }
    gen->store_entries = stores.size();
    return 0;
}
} // namespace


namespace {
// One prime: prepared and published by the calling thread (index, entry table, page-locked output buffer), run either by
// the same thread (mzhip_prime_mem / _file: returns when every entry is decoded) or by a worker thread
// (mzhip_prime_mem_begin: returns at once, readers are served chunk by chunk as the pipeline delivers).
struct PrimeJob {
    const uint8_t *zip = nullptr; // zip[0] = byte `bias` of the archive
    uint64_t zip_len = 0, bias = 0, img_len = 0; // img_len bytes are at hand
    void *own_img = nullptr; // an image this job owns (a rolling window's, from the pinned pool or malloc): given back when the job is done
    size_t own_cap = 0;      // != 0: from the pinned pool
    std::atomic<bool> done{false}; // the worker is through with it (its thread can be joined without waiting)
    ~PrimeJob() {
        if (own_img && own_cap) g_pinned.put(own_img, own_cap);
        else free(own_img);
    }
    int cur = 0; // the device of the thread that asked
    std::vector<int32_t> devs;
    std::shared_ptr<PrimeGen> gen;
    std::vector<int64_t> max_out, wtab;
    std::vector<std::pair<int64_t, int64_t>> stores; /* STORE entries: payload offset, size */
    int64_t result = 0; // entries primed, or the error
    std::string err;
    double t_start = 0;
};
std::mutex g_worker_mu;
// (on the heap and never destroyed: a process that exits with a prime still running must not meet std::terminate in the
// destructor of a joinable thread -- and the HIP runtime may be gone by the time static destructors run)
auto &g_prime_workers = *new std::vector<std::pair<std::thread, std::shared_ptr<PrimeJob>>>();

void prime_unpublish(const std::shared_ptr<PrimeGen> &gen) {
    std::unique_lock<std::shared_mutex> lk(g_prime_mu);
    auto &gens = g_prime.gens;
    for (size_t i = 0; i < gens.size();) {
        if (gens[i] == gen) gens.erase(gens.begin() + (long)i);
        else i++;
    }
    count_store_gens_locked();
}

// lay out a generation for the rows of `table` (8 x int64 each, mzhip_zip_index_mem's; payload offsets known) whose payloads lie
// in the bytes at hand, and publish it with every entry pending.  hash arrays: per row, or null.  0 = nothing to prime.
int64_t prime_publish(const std::shared_ptr<PrimeJob> &job, const int64_t *table, int64_t n, const uint16_t *h_alg, const uint16_t *h_dsz,
                      const uint8_t *h_dig, uint64_t ident, bool window, bool with_stores) {
    const uint8_t *zip = job->zip;
    const uint64_t bias = job->bias, img_end = job->bias + job->img_len;
    std::vector<int64_t> rows; /* the entries a codec kernel can take, in the order their payloads lie in the file */
    for (int64_t i = 0; i < n; i++) {
        const int64_t *t = &table[(size_t)i * 8];
        if ((t[1] & 1) || t[7] < 0 || t[3] < 0 || t[4] < 0 || t[3] >= (1ll << 31) || t[4] >= (1ll << 31) ||
            (uint64_t)t[7] < bias || (uint64_t)t[7] > img_end || (uint64_t)t[3] > img_end - (uint64_t)t[7])
            continue;
        if (with_stores && t[0] == 0 && t[3] == t[4] && t[4] >= (int64_t)MZHIP_CRC_HOST_BELOW) job->stores.emplace_back(t[7], t[4]);
        if (t[0] != 8 && t[0] != 14 && t[0] != 95) continue;
        rows.push_back(i);
    }
    std::stable_sort(rows.begin(), rows.end(), [&](int64_t a, int64_t b) { return table[(size_t)a * 8 + 7] < table[(size_t)b * 8 + 7]; });
    auto gen = std::make_shared<PrimeGen>();
    std::vector<PrimedEntry> &ents = gen->entries;
    ents.reserve(rows.size());
    uint64_t total_out = 0;
    int64_t nseg = 0;
    for (const int64_t i : rows) {
        const int64_t *t = &table[(size_t)i * 8];
        PrimedEntry e;
        memset(&e, 0, sizeof(e));
        e.method = (int32_t)t[0];
        e.payload_off = t[7];
        e.csize = t[3];
        e.usize = t[4];
        e.out_off = (int64_t)total_out;
        e.seg0 = nseg;
        e.status = -1;
        e.head_len = (int32_t)(t[3] < (int64_t)sizeof(e.head) ? t[3] : (int64_t)sizeof(e.head));
        memcpy(e.head, zip + ((uint64_t)t[7] - bias), (size_t)e.head_len);
        if (h_alg && (h_alg[(size_t)i] == 20 || h_alg[(size_t)i] == 23)) { /* SHA-1 / SHA-256: what mz_zip_reader_entry_open sets up (mz_zip_rw.c:414-419) */
            e.hash_alg = h_alg[(size_t)i];
            e.hash_size = h_dsz[(size_t)i];
            memcpy(e.hash_want, &h_dig[(size_t)i * 64], 32);
        }
        ents.push_back(e);
        /* TOTAL_OUT_MAX as mz_zip.c:1833-1846 sets it: the uncompressed size when the EOS flag is set */
        job->max_out.push_back((t[0] != 8 && (t[1] & 2)) ? t[4] : -1);
        job->wtab.insert(job->wtab.end(), t, t + 8);
        total_out += ((uint64_t)t[4] + 15) & ~15ull;
        nseg += (t[4] + kSeg - 1) / kSeg;
    }
    const size_t k = ents.size();
    if (k == 0 && job->stores.empty()) return 0;
    gen->offs.reserve(k);
    for (const PrimedEntry &e : ents) gen->offs.push_back(e.payload_off);
    const double t_idx = prime_now();
    gen->out = (uint8_t *)g_pinned.get(total_out + 16, &gen->out_cap);
    gen->out_pinned = gen->out != nullptr;
    if (!gen->out_pinned) gen->out = (uint8_t *)malloc(total_out + 16);
    if (!gen->out) return -4;
    if (prime_trace())
        fprintf(stderr, "[mzhip prime] %zu entries, %.1f MiB to decode: index %.1f ms, pinned output %.1f ms\n", k,
                (double)total_out / 1048576.0, (t_idx - job->t_start) * 1e3, (prime_now() - t_idx) * 1e3);
    gen->seg_crc.assign((size_t)nseg, 0u);
    gen->state.reset(new std::atomic<uint8_t>[k ? k : 1]);
    for (size_t i = 0; i < k; i++) gen->state[i].store(0, std::memory_order_relaxed);
    gen->zip_len = job->zip_len;
    gen->ident = ident;
    gen->window = window;
    gen->out_bytes = total_out;
    job->gen = gen;
    {
        std::unique_lock<std::shared_mutex> lk(g_prime_mu);
        auto &gens = g_prime.gens;
        for (size_t i = 0; i < gens.size();) { /* a re-prime of the same archive (or window) replaces its generation */
            if (gens[i]->zip_len == gen->zip_len && gens[i]->ident == gen->ident) gens.erase(gens.begin() + (long)i);
            else i++;
        }
        gens.insert(gens.begin(), gen);
        if (gens.size() > kMaxGens) gens.resize(kMaxGens);
        count_store_gens_locked();
    }
    return 1;
}

// index the archive image, lay out the generation and publish it with every entry pending.  0 = nothing to prime.
int64_t prime_prepare(const uint8_t *zip, uint64_t zip_len, const int32_t *devices, int32_t ndev, std::shared_ptr<PrimeJob> *out) {
    auto job = std::make_shared<PrimeJob>();
    job->zip = zip;
    job->zip_len = job->img_len = zip_len;
    job->t_start = prime_now();
    HIP_TRY(hipGetDevice(&job->cur));
    if (ndev <= 0) {
        const int32_t nd = mzhip_device_count();
        if (nd <= 0) return -104;
        for (int32_t d = 0; d < nd; d++) job->devs.push_back(d);
    } else {
        for (int32_t i = 0; i < ndev; i++) job->devs.push_back(devices ? devices[i] : i);
    }
    int64_t n = mzhip_zip_index_mem(zip, zip_len, nullptr, 0);
    if (n <= 0) return n;
    std::vector<int64_t> table((size_t)n * 8);
    mzhip_zip_index_mem(zip, zip_len, table.data(), n);
    std::vector<uint16_t> h_alg((size_t)n), h_dsz((size_t)n);
    std::vector<uint8_t> h_dig((size_t)n * 64);
    if (mzhip_zip_index_hash_mem(zip, zip_len, table.data(), n, h_alg.data(), h_dsz.data(), h_dig.data()) < 0)
        std::fill(h_alg.begin(), h_alg.end(), (uint16_t)0);
    /* identity = length + hash of everything from the first central-directory record to the end of the file */
    const uint64_t cd0 = (uint64_t)table[6];
    const int64_t rc = prime_publish(job, table.data(), n, h_alg.data(), h_dsz.data(), h_dig.data(), fnv1a64(zip + cd0, zip_len - cd0), false, true);
    if (rc <= 0) return rc;
    *out = job;
    return 1;
}

// decode everything the job laid out; every entry leaves the pending state on every way out
void prime_run(const std::shared_ptr<PrimeJob> &job) {
    PrimeGen *gen = job->gen.get();
    const size_t k = gen->entries.size();
    struct Settle {
        PrimeGen *gen;
        size_t k;
        ~Settle() {
            for (size_t i = 0; i < k; i++) {
                uint8_t z = 0;
                (void)gen->state[i].compare_exchange_strong(z, 2);
            }
            { std::lock_guard<std::mutex> lk(gen->mu); }
            gen->cv.notify_all();
        }
    } settle{gen, k};
    const double t0 = prime_now();
    const int32_t world = (int32_t)std::min<size_t>(job->devs.size(), std::max<size_t>(k, 1));
    std::vector<int64_t> bounds((size_t)world + 1);
    mzhip_shard_bounds(job->wtab.data(), (int64_t)k, world, bounds.data());
    std::vector<int32_t> rcs((size_t)world, 0);
    std::vector<std::string> errs((size_t)world);
    auto work = [&](int32_t r) {
        hipError_t he = hipSetDevice(job->devs[(size_t)r]);
        if (he != hipSuccess) rcs[(size_t)r] = fail("hipSetDevice", he);
        else rcs[(size_t)r] = prime_slice(job->zip, job->bias, gen, job->max_out, (size_t)bounds[(size_t)r], (size_t)bounds[(size_t)r + 1]);
        if (rcs[(size_t)r]) errs[(size_t)r] = g_err;
    };
    int now = -1;
    (void)hipGetDevice(&now);
    if (world == 1 && job->devs[0] == now) {
        work(0);
    } else { /* one host thread per device: the host side of the sharded path is C (SURVEY 8e) */
        std::vector<std::thread> th;
        for (int32_t r = 0; r < world; r++) th.emplace_back(work, r);
        for (auto &t : th) t.join();
        (void)hipSetDevice(job->cur);
    }
    for (int32_t r = 0; r < world; r++)
        if (rcs[(size_t)r]) {
            job->err = errs[(size_t)r];
            job->result = rcs[(size_t)r];
            prime_unpublish(job->gen);
            return;
        }
    if (prime_trace()) fprintf(stderr, "[mzhip prime] decode pipeline %.1f ms\n", (prime_now() - t0) * 1e3);
    if (!job->stores.empty()) {
        const int32_t src = prime_store(job->zip, job->bias, job->stores, gen); /* on this thread's device */
        if (src) {
            job->err = g_err;
            job->result = src;
            prime_unpublish(job->gen);
            return;
        }
        gen->store_ready.store(true, std::memory_order_release);
        std::unique_lock<std::shared_mutex> lk(g_prime_mu);
        count_store_gens_locked();
    }
    int64_t good = 0;
    for (size_t i = 0; i < k; i++) good += gen->state[i].load(std::memory_order_relaxed) == 1 ? 1 : 0;
    job->result = good + (int64_t)gen->store_entries;
}

// A process may exit while a prime is still running (a look-ahead window nobody came to read, an application that stops early):
// the HIP runtime's own teardown must not meet a worker in the middle of a copy.  The first worker that is started registers this
// handler; it runs before the runtime's (registered when the runtime was loaded, i.e. earlier: LIFO): the imaging threads of
// shim_autoprime.c finish the window they are reading and take no other, then every decode worker is joined.
extern "C" void mzhip_autoprime_quiesce(void) __attribute__((weak));
int64_t prime_wait_all();
void prime_at_exit() {
    if (mzhip_autoprime_quiesce) mzhip_autoprime_quiesce();
    (void)prime_wait_all();
}
void prime_register_exit() {
    static std::once_flag once;
    std::call_once(once, [] { (void)atexit(prime_at_exit); });
}

// join the workers that are through (a process that rolls over a large archive starts one per window); g_worker_mu is held.
// Their results stay with prime_wait_all()'s tally only while they are listed, so a failed one is kept for it to report.
void prime_reap_locked() {
    for (size_t i = 0; i < g_prime_workers.size();) {
        auto &w = g_prime_workers[i];
        if (w.second->done.load(std::memory_order_acquire) && w.second->result >= 0 && w.second->gen && w.second->gen->window) {
            if (w.first.joinable()) w.first.join();
            g_prime_workers.erase(g_prime_workers.begin() + (long)i);
        } else {
            i++;
        }
    }
}

int64_t prime_wait_all() {
    std::vector<std::pair<std::thread, std::shared_ptr<PrimeJob>>> w;
    {
        std::lock_guard<std::mutex> lk(g_worker_mu);
        w.swap(g_prime_workers);
    }
    int64_t total = 0, bad = 0;
    for (auto &p : w) {
        if (p.first.joinable()) p.first.join();
        if (p.second->result < 0) {
            if (!bad) {
                bad = p.second->result;
                snprintf(g_err, sizeof(g_err), "%s", p.second->err.c_str());
            }
        } else {
            total += p.second->result;
        }
    }
    return bad ? bad : total;
}
} // namespace

extern "C" {

int64_t mzhip_prime_mem_multi(const uint8_t *zip, uint64_t zip_len, const int32_t *devices, int32_t ndev) {
    std::shared_ptr<PrimeJob> job;
    const int64_t rc = prime_prepare(zip, zip_len, devices, ndev, &job);
    if (rc <= 0) return rc;
    prime_run(job);
    if (job->result < 0) snprintf(g_err, sizeof(g_err), "%s", job->err.c_str());
    return job->result;
}

int64_t mzhip_prime_mem(const uint8_t *zip, uint64_t zip_len) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const int32_t d = (int32_t)cur;
    return mzhip_prime_mem_multi(zip, zip_len, &d, 1);
}

int64_t mzhip_prime_mem_begin(const uint8_t *zip, uint64_t zip_len) {
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    const int32_t d = (int32_t)cur;
    std::shared_ptr<PrimeJob> job;
    const int64_t rc = prime_prepare(zip, zip_len, &d, 1, &job);
    if (rc <= 0) return rc;
    const int64_t n = (int64_t)job->gen->entries.size() + (int64_t)job->stores.size();
    try {
        prime_register_exit();
        std::lock_guard<std::mutex> lk(g_worker_mu);
        prime_reap_locked();
        g_prime_workers.emplace_back(std::thread([job] {
                                         (void)hipSetDevice(job->cur);
                                         (void)mzhip_bind_thread_near_device(job->cur, 0); /* this thread feeds the copy engines: next to the device */
                                         prime_run(job);
                                         job->done.store(true, std::memory_order_release);
                                     }),
                                     job);
    } catch (...) { /* no thread to be had: the entries must not stay pending -- decode here and now */
        prime_run(job);
        if (job->result < 0) {
            snprintf(g_err, sizeof(g_err), "%s", job->err.c_str());
            return job->result;
        }
    }
    return n;
}

int64_t mzhip_prime_wait(void) {
    const int64_t r = prime_wait_all();
    if (prime_trace() && g_prime_wait_n.load())
        fprintf(stderr, "[mzhip prime] %llu lookups waited for their chunk, %.1f ms in all\n", (unsigned long long)g_prime_wait_n.exchange(0),
                (double)g_prime_wait_ns.exchange(0) * 1e-6);
    return r;
}

/* ---- one WINDOW of an archive that is rolled over (shim_autoprime.c; not part of the public ABI) ----
 * img[0 .. win_len) = bytes [win_off, win_off + win_len) of an archive of zip_len bytes; rows = n rows of 8 (payload offsets
 * resolved, mzhip_zip_index_resolve) with their Hash fields or NULLs.  The call takes the image over -- img_cap != 0: it came
 * from mzhip_window_alloc and goes back there, 0: malloc -- on every way out, publishes a generation of its own for the window
 * (identity zip_len + ident) with every entry pending and decodes it on `device` (-1: the calling thread's) on a worker thread: readers are served chunk by chunk as
 * the pipeline delivers, as under mzhip_prime_mem_begin.  STORE entries are not kept (the raw stream serves them).  Returns the
 * entries published, 0 = none (nothing was published), < 0 = an MZ_* code.  *out_bytes: bytes of the cache the generation's entries take. */
__attribute__((visibility("hidden"))) int64_t mzhip_prime_window_begin(uint8_t *img, size_t img_cap, uint64_t win_off, uint64_t win_len,
                                                                       const int64_t *rows, int64_t n, const uint16_t *alg,
                                                                       const uint16_t *dsz, const uint8_t *dig, uint64_t zip_len,
                                                                       uint64_t ident, int32_t device, uint64_t *out_bytes) {
    auto job = std::make_shared<PrimeJob>();
    job->own_img = img;
    job->own_cap = img_cap;
    job->zip = img;
    job->zip_len = zip_len;
    job->bias = win_off;
    job->img_len = win_len;
    job->t_start = prime_now();
    if (out_bytes) *out_bytes = 0;
    if (!img || !rows || n <= 0) return 0;
    if (device >= 0) { /* (the imaging thread of shim_autoprime.c works for readers on any device) */
        HIP_TRY(hipSetDevice(device));
        job->cur = device;
    } else {
        HIP_TRY(hipGetDevice(&job->cur));
    }
    job->devs.push_back((int32_t)job->cur);
    const int64_t rc = prime_publish(job, rows, n, alg, dsz, dig, ident, true, false);
    if (rc <= 0) return rc;
    const int64_t k = (int64_t)job->gen->entries.size();
    if (out_bytes) *out_bytes = job->gen->out_bytes;
    try {
        prime_register_exit();
        std::lock_guard<std::mutex> lk(g_worker_mu);
        prime_reap_locked();
        g_prime_workers.emplace_back(std::thread([job] {
                                         (void)hipSetDevice(job->cur);
                                         (void)mzhip_bind_thread_near_device(job->cur, 0);
                                         prime_run(job);
                                         if (job->own_img) { /* the image is done with once the last H2D copy has been waited for */
                                             if (job->own_cap) g_pinned.put(job->own_img, job->own_cap);
                                             else free(job->own_img);
                                             job->own_img = nullptr;
                                         }
                                         job->done.store(true, std::memory_order_release);
                                     }),
                                     job);
    } catch (...) {
        prime_run(job);
        if (job->result < 0) {
            snprintf(g_err, sizeof(g_err), "%s", job->err.c_str());
            return job->result;
        }
    }
    return k;
}
/* drop the generation of that identity (streams that read from it keep it alive until they let go) */
__attribute__((visibility("hidden"))) void mzhip_prime_drop(uint64_t zip_len, uint64_t ident) {
    std::shared_ptr<PrimeGen> victim; /* (freed outside the lock) */
    {
        std::unique_lock<std::shared_mutex> lk(g_prime_mu);
        auto &gens = g_prime.gens;
        for (size_t i = 0; i < gens.size(); i++)
            if (gens[i]->zip_len == zip_len && gens[i]->ident == ident) {
                victim = gens[i];
                gens.erase(gens.begin() + (long)i);
                break;
            }
        count_store_gens_locked();
    }
}
/* is that generation still published?  (kMaxGens, a clear or a re-prime may have taken it)  ident 0: is ANY whole image of that
 * length published -- the application primed the archive itself */
__attribute__((visibility("hidden"))) int32_t mzhip_prime_has(uint64_t zip_len, uint64_t ident) {
    std::shared_lock<std::shared_mutex> lk(g_prime_mu);
    for (const auto &g : g_prime.gens)
        if (g->zip_len == zip_len && (ident ? g->ident == ident : !g->window)) return 1;
    return 0;
}
__attribute__((visibility("hidden"))) uint64_t mzhip_prime_clears(void) { return g_prime_clears.load(std::memory_order_relaxed); }
__attribute__((visibility("hidden"))) int32_t mzhip_prime_current_device(void) {
    int d = 0;
    return hipGetDevice(&d) == hipSuccess ? (int32_t)d : -1;
}
/* generations published now: all of them / the windows among them; clears so far */
__attribute__((visibility("hidden"))) void mzhip_prime_counts(int32_t *gens, int32_t *windows, uint64_t *clears) {
    std::shared_lock<std::shared_mutex> lk(g_prime_mu);
    int32_t w = 0;
    for (const auto &g : g_prime.gens) w += g->window ? 1 : 0;
    if (gens) *gens = (int32_t)g_prime.gens.size();
    if (windows) *windows = w;
    if (clears) *clears = g_prime_clears.load(std::memory_order_relaxed);
}

static int64_t prime_file_on(const char *path, const int32_t *devices, int32_t ndev, int multi) {
    FILE *f = fopen(path, "rb");
    if (!f) return -111; /* MZ_OPEN_ERROR */
    fseeko(f, 0, SEEK_END);
    const int64_t len = (int64_t)ftello(f);
    fseeko(f, 0, SEEK_SET);
    const double t0 = prime_now();
    size_t cap = 0;
    uint8_t *buf = (uint8_t *)g_pinned.get((size_t)(len > 0 ? len : 1), &cap); /* page-locked: the H2D copies of the payload ranges run at link speed */
    const bool pinned = buf != nullptr;
    if (!pinned) buf = (uint8_t *)malloc((size_t)(len > 0 ? len : 1));
    const double t1 = prime_now();
    int64_t rc = -115; /* MZ_READ_ERROR */
    const bool got = buf && len > 0 && fread(buf, 1, (size_t)len, f) == (size_t)len;
    const double t2 = prime_now();
    if (got) rc = multi ? mzhip_prime_mem_multi(buf, (uint64_t)len, devices, ndev) : mzhip_prime_mem(buf, (uint64_t)len);
    if (prime_trace())
        fprintf(stderr, "[mzhip prime] %s: %.1f MiB image: pinned buffer %.1f ms, read %.1f ms, prime %.1f ms\n", path,
                (double)len / 1048576.0, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (prime_now() - t2) * 1e3);
    if (pinned) g_pinned.put(buf, cap);
    else free(buf);
    fclose(f);
    return rc;
}

int64_t mzhip_prime_file_multi(const char *path, const int32_t *devices, int32_t ndev) { return prime_file_on(path, devices, ndev, 1); }

int64_t mzhip_prime_file(const char *path) { return prime_file_on(path, nullptr, 0, 0); }

void mzhip_prime_hash_stats(uint64_t *checked, uint64_t *mismatched) {
    if (checked) *checked = g_prime_hash_checked.load();
    if (mismatched) *mismatched = g_prime_hash_bad.load();
}

void mzhip_prime_stats(uint64_t *entries, uint64_t *hits, uint64_t *misses) {
    std::shared_lock<std::shared_mutex> lk(g_prime_mu);
    if (entries) {
        *entries = 0;
        for (const auto &g : g_prime.gens) {
            for (size_t i = 0; i < g->entries.size(); i++) *entries += g->state[i].load(std::memory_order_relaxed) == 1 ? 1 : 0;
            *entries += g->store_entries;
        }
    }
    if (hits) *hits = g_prime_hits.load();
    if (misses) *misses = g_prime_misses.load();
}

// Used by mz_crypt_crc32_update: are these `size` bytes a chunk of a primed STORE entry?  The fingerprint finds the
// candidates, memcmp against the kept payload decides (so a file that changed between the prime and the read is
// never answered with the old CRC).  1 = yes, *crc = the chunk's CRC-32 as the device computed it.
__attribute__((visibility("hidden"))) int32_t mzhip_prime_store_crc(const uint8_t *buf, int32_t size, uint32_t *crc) {
    if (g_store_gens.load(std::memory_order_relaxed) == 0 || size < 32 || (uint32_t)size > kSeg) return 0;
    std::vector<std::shared_ptr<PrimeGen>> gens;
    {
        std::shared_lock<std::shared_mutex> lk(g_prime_mu);
        gens = g_prime.gens; /* the generations are immutable once published: search them without the lock */
    }
    const uint64_t key = store_key(buf, (uint32_t)size);
    for (const std::shared_ptr<PrimeGen> &g : gens) {
        if (!g->store_ready.load(std::memory_order_acquire)) continue; /* (its STORE index is still being built) */
        auto range = g->store_idx.equal_range(key);
        for (auto it = range.first; it != range.second; ++it) {
            const PrimeGen::StoreSeg &sg = g->store_segs[it->second];
            if (sg.len == (uint32_t)size && memcmp(buf, g->store + sg.off, (size_t)size) == 0) {
                *crc = sg.crc;
                g_prime_hits.fetch_add(1, std::memory_order_relaxed);
                return 1;
            }
        }
    }
    return 0;
}

__attribute__((visibility("hidden"))) int32_t mzhip_prime_any(void) { return g_any_gens.load(std::memory_order_relaxed) != 0; }

// Used by the READ shims: is the entry whose payload starts at `payload_off` primed?  The stream presents the payload
// bytes it has pulled so far (`head`, at least min(csize, 16) of them) and, when the zip layer set one, its
// TOTAL_IN_MAX (= the entry's compressed size, mz_zip.c:1829); offset, method, compressed size and up to 256 leading
// payload bytes must all agree.  On a hit returns 1, the cached output / sizes / CRCs, and *pin: a reference that keeps
// the generation alive until the stream hands it back with mzhip_prime_unpin() (close / delete / re-open).
__attribute__((visibility("hidden"))) int32_t mzhip_prime_lookup3(int32_t method, int64_t payload_off, const uint8_t *head,
                                                                  int32_t head_len, int64_t max_total_in, const uint8_t **data,
                                                                  int64_t *usize, int64_t *csize, uint32_t *crc,
                                                                  const uint32_t **seg_crc, void **pin, uint16_t *hash_alg,
                                                                  const uint8_t **hash_digest) {
    *pin = nullptr;
    if (hash_alg) *hash_alg = 0;
    if (hash_digest) *hash_digest = nullptr;
    std::vector<std::shared_ptr<PrimeGen>> gens;
    {
        std::shared_lock<std::shared_mutex> lk(g_prime_mu);
        if (g_prime.gens.empty()) return 0;
        gens = g_prime.gens; /* the keys of a published generation never change: search (and wait) without the lock */
    }
    /* the entry of generation g that this stream could be, settled (its chunk of the decode pipeline has landed): its
     * index, or -1.  What a stream can present is where its payload starts, the codec, the compressed size the zip
     * layer told it and the first bytes it pulled. */
    auto candidate = [&](const std::shared_ptr<PrimeGen> &g) -> int64_t {
        const std::vector<PrimedEntry> &ents = g->entries;
        const std::vector<int64_t> &offs = g->offs;
        if (offs.empty() || payload_off < offs.front() || payload_off > offs.back()) return -1;
        size_t lo = 0, hi = offs.size();
        while (lo < hi) {
            size_t mid = (lo + hi) / 2;
            if (offs[mid] < payload_off) lo = mid + 1; else hi = mid;
        }
        if (lo == offs.size() || offs[lo] != payload_off) return -1;
        const PrimedEntry &e = ents[lo];
        const int32_t need = e.head_len < 16 ? e.head_len : 16;
        const int32_t cmp = head_len < e.head_len ? head_len : e.head_len;
        if (e.method != method || head_len < need || memcmp(head, e.head, (size_t)cmp) != 0) return -1;
        if (max_total_in > 0 && max_total_in != e.csize) return -1;
        if (g->state) { /* the entry's chunk may still be on its way: wait for that chunk */
            if (g->state[lo].load(std::memory_order_acquire) == 0) {
                const double w0 = prime_trace() ? prime_now() : 0.0;
                {
                    std::unique_lock<std::mutex> lk(g->mu);
                    g->cv.wait(lk, [&] { return g->state[lo].load(std::memory_order_acquire) != 0; });
                }
                if (prime_trace()) {
                    g_prime_wait_ns.fetch_add((uint64_t)((prime_now() - w0) * 1e9), std::memory_order_relaxed);
                    g_prime_wait_n.fetch_add(1, std::memory_order_relaxed);
                }
            }
            if (g->state[lo].load(std::memory_order_acquire) != 1) return -1; /* did not decode to its declared sizes: the ordinary path has the verdict */
        }
        return (int64_t)lo;
    };
    for (size_t gi = 0; gi < gens.size(); gi++) {
        const std::shared_ptr<PrimeGen> &g = gens[gi];
        const int64_t at = candidate(g);
        if (at < 0) continue;
        const PrimedEntry &e = g->entries[(size_t)at];
        /* Several archives may be primed at once (two versions of one file ...), and entries of two of them can agree in
         * everything a stream presents while their payloads differ past the 256th byte.  Then nobody can say whose
         * stream this is: it is not served (the ordinary per-entry path decodes what the stream really holds). */
        bool ambiguous = false;
        for (size_t gj = gi + 1; gj < gens.size() && !ambiguous; gj++) {
            const int64_t o = candidate(gens[gj]);
            if (o < 0) continue;
            const PrimedEntry &f = gens[gj]->entries[(size_t)o];
            ambiguous = f.crc != e.crc || f.usize != e.usize;
        }
        if (ambiguous) break;
        *data = g->out + e.out_off;
        *usize = e.usize;
        *csize = e.csize;
        *crc = e.crc;
        *seg_crc = g->seg_crc.data() + e.seg0;
        if (e.hash_alg && hash_alg && hash_digest) { /* (served, so the device's digest is the Hash field's) */
            *hash_alg = e.hash_alg;
            *hash_digest = e.hash_got;
        }
        g_prime_hits.fetch_add(1, std::memory_order_relaxed);
        *pin = new std::shared_ptr<PrimeGen>(g);
        return 1;
    }
    g_prime_misses.fetch_add(1, std::memory_order_relaxed);
    if (prime_trace()) {
        /* why: no generation knows the offset / one does but the stream's facts differ / its entry was not servable */
        int known = 0, unserv = 0;
        for (const auto &g : gens) {
            const std::vector<PrimedEntry> &ents = g->entries;
            size_t lo = 0, hi = ents.size();
            while (lo < hi) {
                size_t mid = (lo + hi) / 2;
                if (ents[mid].payload_off < payload_off) lo = mid + 1; else hi = mid;
            }
            if (lo < ents.size() && ents[lo].payload_off == payload_off) {
                known++;
                if (g->state && g->state[lo].load(std::memory_order_acquire) == 2) unserv++;
                fprintf(stderr, "[mzhip prime] miss at payload %lld: generation %s knows it (method %d / %d, csize %lld / max_in %lld, head %d / %d, state %d, status %d)\n",
                        (long long)payload_off, g->window ? "(window)" : "(whole)", ents[lo].method, method, (long long)ents[lo].csize, (long long)max_total_in,
                        ents[lo].head_len, head_len, g->state ? (int)g->state[lo].load() : -1, ents[lo].status);
            }
        }
        if (!known) fprintf(stderr, "[mzhip prime] miss at payload %lld (method %d): no generation of %zu knows the offset\n", (long long)payload_off, method, gens.size());
        (void)unserv;
    }
    return 0;
}

__attribute__((visibility("hidden"))) void mzhip_prime_unpin(void *pin) {
    if (!pin) return;
    delete (std::shared_ptr<PrimeGen> *)pin; // (the last reference frees the generation: its buffers go back to pools with locks of their own)
}

// checksums only: crc(A||B) from crc(A), crc(B), |B| (shared with shim_crc32.c)
__attribute__((visibility("hidden"))) uint32_t mzhip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return mzhip_crc32_combine_host(crc_a, crc_b, len_b);
}

} // extern "C"
