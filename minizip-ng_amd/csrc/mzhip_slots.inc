// mzhip_slots.inc -- the event-guarded slot pool behind every kernel launch, once, and its two users: the cache of per-launch
// device scratch and the cache of work-queue heads, each with its RAII lease.  Two parts:
//   declarations (always): what mzhip_runtime.h shows both halves of the runtime -- the records and the leases;
//   definitions (with MZHIP_SLOTS_DEFINE, in ONE translation unit: mzhip_launch.inc's): the lock, the pool, the leases' bodies.
// It names only the runtime API (hipEvent*, hipMalloc / hipFree, hipMemsetAsync, hipStreamPerThread) and HIP_TRY / g_err of
// mzhip_runtime.h, so tests/unit_slot_cache.cpp compiles it over a stand-in and drives it on a CPU.
//
// The rule, for both caches: a slot may be handed out again when the next user is on the stream that used it last (stream order
// protects it) or when the event recorded behind its last use has completed; otherwise another slot is taken, and with every
// slot busy on other streams one is taken and its last launch waited for -- outside the lock, the slot marked `held` under it.
#ifndef MZHIP_SLOTS_DECLARED
#define MZHIP_SLOTS_DECLARED

#include <stddef.h>
#include <stdint.h>

#define MZ_NUM_COUNTERS 64 // (mzhip_kernels.hip says the same ahead of its kernels; a different number there would not compile quietly)

namespace mzh {

struct Slot {
    hipEvent_t ev = nullptr;    // recorded behind the last launch that used the slot (made once, never destroyed: mzhip_prime.inc, g_lane_sets)
    hipStream_t last = nullptr; // ... on this stream (stream_key)
    bool used = false;          // `ev` has been recorded
    bool held = false;          // leased right now: nobody else's
};

// Per-launch device scratch (K1's records, K4 / K6 tokens, ...) and the staging of the host-buffer calls, stream-ordered
// without the runtime's memory pools.  hipMallocAsync/hipFreeAsync was the first implementation; on this stack (ROCm 7.2,
// gfx950) the second allocation of a process intermittently came back with the kernels' and copies' early writes wiped (the
// whole block read as zero afterwards: 16 of 100 fresh processes, profiles/r1/side_measurements.log), so buffers are plain
// hipMalloc memory cached here: best fit among the reusable ones, else a new one (2 MiB granules) in an empty slot or in
// place of an idle one that is too small, so concurrent streams never share scratch.
constexpr int kScratchSlots = 32;
struct ScratchCache {
    Slot slot[kScratchSlots];
    void *p[kScratchSlots] = {};
    size_t cap[kScratchSlots] = {};
};
struct ScratchLease {
    ScratchCache *cache = nullptr;
    hipStream_t s = nullptr;
    int slot = -1;
    void *p = nullptr;
    int32_t get(ScratchCache *from, size_t bytes, hipStream_t st);
    int32_t release(); // records the event behind what was queued on `s`; the destructor does the same for every early return
    ~ScratchLease() { (void)release(); }
};

// The work-queue heads of one launch: two words per slot (the LZMA decoder's two kernels each have a head), zeroed on the
// lease's stream.  The batch entry points are asynchronous on caller-supplied streams, hence the same rule; the search starts
// behind the slot handed out last.
struct CounterCache {
    Slot slot[MZ_NUM_COUNTERS];
    uint32_t next = 0;
    uint32_t *words = nullptr; // 2 * MZ_NUM_COUNTERS of them on the device
};
struct CounterLease {
    CounterCache *cache = nullptr;
    hipStream_t s = nullptr;
    int idx = -1;
    uint32_t *p = nullptr;
    int32_t get(CounterCache *from, hipStream_t st);
    ~CounterLease();
};

} // namespace mzh
#endif

#if defined(MZHIP_SLOTS_DEFINE) && !defined(MZHIP_SLOTS_DEFINED)
#define MZHIP_SLOTS_DEFINED

#include <mutex>
#include <stdio.h>

namespace mzh {
namespace {

std::mutex g_mu; // device-wide: the table of device contexts and both caches of every device

// Identity of a stream for the "same stream => stream order protects the slot" shortcut.  hipStreamPerThread is ONE handle
// value that names a different stream in every host thread: two threads must not take each other for the same stream (they
// did for a day: a second thread's launch reused the work-queue head and the record scratch of a kernel that was still
// running -- CRC errors in the two-thread drop-in test).
hipStream_t stream_key(hipStream_t s) {
    static thread_local char tls_marker;
    return s == hipStreamPerThread ? (hipStream_t)(void *)&tls_marker : s;
}

// (all three under g_mu)  is the launch that used the slot last over? / may the stream with this key have the slot now?
bool slot_idle(const Slot &e) { return !e.used || hipEventQuery(e.ev) == hipSuccess; }
bool slot_reusable(const Slot &e, hipStream_t key) { return !e.held && (!e.used || e.last == key || hipEventQuery(e.ev) == hipSuccess); }
// Take slot `i`, the cache's choice -- or, with i < 0 (nothing reusable: every slot is busy on another stream), the first one
// from `start` that nobody is setting up right now; *wait_for is then the event of its last launch, which the caller waits
// for AFTER unlocking: one thread waiting for a slot must not stall every other thread's launches (ADVICE r2).
int32_t slot_take(Slot *slot, int n, uint32_t start, int i, const char *all_held, int *taken, hipEvent_t *wait_for) {
    for (int k = 0; k < n && i < 0; k++) {
        const int j = (int)((start + (uint32_t)k) % (uint32_t)n);
        if (slot[j].held) continue;
        i = j;
        if (slot[j].used) *wait_for = slot[j].ev;
    }
    if (i < 0) {
        snprintf(g_err, sizeof(g_err), all_held, n);
        return -104;
    }
    if (!slot[i].ev) HIP_TRY(hipEventCreateWithFlags(&slot[i].ev, hipEventDisableTiming));
    slot[i].held = true; /* the lease's from here on */
    *taken = i;
    return 0;
}
int32_t slot_give_back(Slot &e, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_mu);
    e.held = false;
    e.used = true;
    e.last = stream_key(s);
    HIP_TRY(hipEventRecord(e.ev, s));
    return 0;
}

} // namespace

int32_t ScratchLease::get(ScratchCache *from, size_t bytes, hipStream_t st) {
    ScratchCache &c = *from;
    hipEvent_t wait_for = nullptr;
    int best = -1;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const hipStream_t key = stream_key(st);
        int empty = -1, victim = -1;
        for (int i = 0; i < kScratchSlots; i++) {
            if (c.slot[i].held) continue;
            if (!c.p[i]) {
                if (empty < 0) empty = i;
            } else if (c.cap[i] >= bytes && slot_reusable(c.slot[i], key)) {
                if (best < 0 || c.cap[i] < c.cap[best]) best = i;
            } else if (c.cap[i] < bytes && slot_idle(c.slot[i]) && (victim < 0 || c.cap[i] < c.cap[victim])) {
                victim = i; // idle and too small
            }
        }
        const int32_t rc = slot_take(c.slot, kScratchSlots, 0, best >= 0 ? best : empty >= 0 ? empty : victim,
                                     "scratch: more than %d concurrent launches", &slot, &wait_for);
        if (rc) return rc;
    }
    cache = from;
    s = st;
    if (wait_for) HIP_TRY(hipEventSynchronize(wait_for));
    if (slot != best) { /* a new buffer in this slot (held: nobody else looks at it) */
        std::lock_guard<std::mutex> lk(g_mu);
        if (c.p[slot]) {
            HIP_TRY(hipFree(c.p[slot]));
            c.p[slot] = nullptr;
            c.cap[slot] = 0;
        }
        const size_t cap = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        HIP_TRY(hipMalloc(&c.p[slot], cap));
        c.cap[slot] = cap;
        c.slot[slot].used = false;
    }
    p = c.p[slot];
    return 0;
}

int32_t ScratchLease::release() {
    if (slot < 0) return 0;
    Slot &e = cache->slot[slot];
    slot = -1;
    return slot_give_back(e, s);
}

int32_t CounterLease::get(CounterCache *from, hipStream_t st) {
    hipEvent_t wait_for = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const hipStream_t key = stream_key(st);
        int i = -1;
        for (uint32_t k = 0; k < MZ_NUM_COUNTERS && i < 0; k++) {
            const uint32_t j = (from->next + k) % MZ_NUM_COUNTERS;
            if (slot_reusable(from->slot[j], key)) i = (int)j;
        }
        const int32_t rc = slot_take(from->slot, MZ_NUM_COUNTERS, from->next, i, "more than %d launches being set up at once", &idx, &wait_for);
        if (rc) return rc;
        from->next = (uint32_t)idx + 1u;
    }
    cache = from;
    s = st;
    if (wait_for) HIP_TRY(hipEventSynchronize(wait_for));
    p = from->words + 2 * idx;
    HIP_TRY(hipMemsetAsync(p, 0, 2 * sizeof(uint32_t), s));
    return 0;
}

CounterLease::~CounterLease() {
    if (idx >= 0) (void)slot_give_back(cache->slot[idx], s);
}

} // namespace mzh
#endif
