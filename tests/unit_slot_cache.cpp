// The scratch and work-queue caches of the runtime (minizip-ng_amd/csrc/mzhip_slots.inc) on a CPU: the file is compiled over
// the stand-in below, in which the TEST decides when an event has completed and allocations are counted (built and run by
// tests/test_kernel_emul.py::test_slot_cache_rules; also the program to build with -fsanitize=thread / address,undefined).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// ---- stand-in for the runtime API: events complete when the test says so, device memory is a number
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorNotReady = 600 };
enum { hipEventDisableTiming = 2 };
typedef struct FakeStream *hipStream_t;
#define hipStreamPerThread ((hipStream_t)2)
static hipStream_t stream(int i) { return (hipStream_t)(uintptr_t)(0x1000 + 16 * i); }

struct FakeEvent {
    std::atomic<bool> done{true};
    std::atomic<hipStream_t> on{nullptr};
    std::atomic<int> records{0};
};
typedef FakeEvent *hipEvent_t;
static FakeEvent g_events[1024]; // (never destroyed, as in the product; no heap, so a leak checker has nothing to say)
static std::atomic<int> g_nevents{0};
static std::mutex g_ev_mu;
static std::condition_variable g_ev_cv;
static std::atomic<int> g_in_wait{0}; // threads inside hipEventSynchronize

static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    *e = &g_events[g_nevents++];
    return hipSuccess;
}
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    e->done = false;
    e->on = s;
    e->records++;
    return hipSuccess;
}
static hipError_t hipEventQuery(hipEvent_t e) { return e->done ? hipSuccess : hipErrorNotReady; }
static hipError_t hipEventSynchronize(hipEvent_t e) {
    std::unique_lock<std::mutex> lk(g_ev_mu);
    g_in_wait++;
    g_ev_cv.wait(lk, [&] { return e->done.load(); });
    g_in_wait--;
    return hipSuccess;
}
static void complete(hipEvent_t e) {
    std::lock_guard<std::mutex> lk(g_ev_mu);
    e->done = true;
    g_ev_cv.notify_all();
}

static char g_arena[4096]; // a "device pointer" is the address of one of these bytes
static size_t g_size[4096];
static std::mutex g_mem_mu;
static int g_live = 0, g_max_live = 0, g_mallocs = 0, g_frees = 0;
static hipError_t hipMalloc(void **p, size_t n) {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    for (int i = 0; i < 4096; i++)
        if (!g_size[i]) {
            g_size[i] = n;
            *p = &g_arena[i];
            g_mallocs++;
            if (++g_live > g_max_live) g_max_live = g_live;
            return hipSuccess;
        }
    return 2;
}
static hipError_t hipFree(void *p) {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    g_size[(char *)p - g_arena] = 0;
    g_live--;
    g_frees++;
    return hipSuccess;
}
static size_t size_of(void *p) {
    std::lock_guard<std::mutex> lk(g_mem_mu);
    return g_size[(char *)p - g_arena];
}
struct {
    void *p;
    size_t n;
    hipStream_t s;
} g_last_memset;
static hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t s) {
    memset(p, v, n);
    std::lock_guard<std::mutex> lk(g_mem_mu);
    g_last_memset = {p, n, s};
    return hipSuccess;
}

namespace mzh {
thread_local char g_err[256] = "";
int32_t fail(const char *what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s failed (%d)", what, e);
    return -104;
}
} // namespace mzh
#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return mzh::fail(#expr, _e); \
    } while (0)

#define MZHIP_SLOTS_DEFINE
#include "../minizip-ng_amd/csrc/mzhip_slots.inc"
using namespace mzh;

// ---- the checks
static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        g_checks++;                                                     \
        if (!(cond)) {                                                  \
            g_failed++;                                                 \
            printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);     \
        }                                                               \
    } while (0)
static const size_t MiB = (size_t)1 << 20;

static bool wait_until(const std::function<bool()> &f) { // at most 10 s
    const auto end = std::chrono::steady_clock::now() + std::chrono::seconds(10);
    while (!f()) {
        if (std::chrono::steady_clock::now() > end) return false;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    return true;
}
static void complete_all(Slot *slot, int n) {
    for (int i = 0; i < n; i++)
        if (slot[i].ev) complete(slot[i].ev);
}

static void same_and_other_stream() { // 1, 2
    static ScratchCache c;
    ScratchLease a;
    CHECK(a.get(&c, 1000, stream(1)) == 0 && a.slot >= 0 && a.p);
    const int first = a.slot;
    CHECK(size_of(a.p) == 2 * MiB);
    CHECK(a.release() == 0 && a.slot < 0);
    CHECK(c.slot[first].used && !c.slot[first].held && !c.slot[first].ev->done);
    {
        ScratchLease b; /* the stream that used it last: stream order protects the buffer */
        const int before = g_mallocs;
        CHECK(b.get(&c, 1000, stream(1)) == 0 && b.slot == first && g_mallocs == before);
    }
    ScratchLease other;
    CHECK(other.get(&c, 1000, stream(2)) == 0 && other.slot != first);
    complete(c.slot[first].ev);
    ScratchLease third;
    CHECK(third.get(&c, 1000, stream(3)) == 0 && third.slot == first);
}

static void best_fit() { // 3
    static ScratchCache c;
    int slot4 = -1;
    void *p4 = nullptr;
    {
        ScratchLease a, b, d;
        CHECK(a.get(&c, 8 * MiB, stream(1)) == 0 && b.get(&c, 2 * MiB, stream(1)) == 0 && d.get(&c, 4 * MiB - 5, stream(1)) == 0);
        slot4 = d.slot;
        p4 = d.p;
    }
    complete_all(c.slot, kScratchSlots);
    const int before = g_mallocs;
    ScratchLease l;
    CHECK(l.get(&c, 3 * MiB, stream(2)) == 0 && l.slot == slot4 && l.p == p4 && size_of(l.p) == 4 * MiB && g_mallocs == before);
}

static void replace_small_idle() { // 4
    static ScratchCache c;
    const int live0 = g_live;
    g_max_live = g_live;
    {
        ScratchLease l[kScratchSlots];
        for (int i = 0; i < kScratchSlots; i++) CHECK(l[i].get(&c, 1 + (size_t)i * 1000, stream(1)) == 0);
    }
    CHECK(g_live - live0 == kScratchSlots);
    complete_all(c.slot, kScratchSlots);
    const int frees = g_frees;
    ScratchLease big;
    CHECK(big.get(&c, 5 * MiB, stream(2)) == 0 && size_of(big.p) == 6 * MiB);
    CHECK(g_frees == frees + 1 && g_live - live0 == kScratchSlots && g_max_live - live0 == kScratchSlots);
    for (int i = 0; i < kScratchSlots; i++) CHECK(c.p[i] && c.cap[i] == size_of(c.p[i]) && c.cap[i] % (2 * MiB) == 0);
}

static void stream_per_thread() { // 5
    static ScratchCache c;
    static CounterCache cc;
    static uint32_t words[2 * MZ_NUM_COUNTERS];
    cc.words = words;
    hipStream_t key[2] = {nullptr, nullptr};
    int slot[3] = {-1, -1, -1}, head[2] = {-1, -1};
    std::atomic<int> step{0};
    std::thread t1([&] {
        key[0] = stream_key(hipStreamPerThread);
        ScratchLease l;
        if (l.get(&c, 1000, hipStreamPerThread) == 0) slot[0] = l.slot;
        (void)l.release();
        ScratchLease again;
        if (again.get(&c, 1000, hipStreamPerThread) == 0) slot[2] = again.slot;
        for (int i = 0; i < MZ_NUM_COUNTERS; i++) { /* every head used last by this thread's stream, none completed */
            CounterLease h;
            if (h.get(&cc, hipStreamPerThread) != 0) head[0] = -2;
        }
        step = 1;
        while (step != 2) std::this_thread::sleep_for(std::chrono::milliseconds(1)); /* (alive to the end: its TLS is not handed on) */
    });
    CHECK(wait_until([&] { return step == 1; }));
    std::thread t2([&] {
        key[1] = stream_key(hipStreamPerThread);
        ScratchLease l;
        if (l.get(&c, 1000, hipStreamPerThread) == 0) slot[1] = l.slot;
        head[1] = g_in_wait; /* (nothing waits yet) */
    });
    t2.join();
    CHECK(key[0] && key[1] && key[0] != key[1] && key[0] != hipStreamPerThread);
    CHECK(stream_key(stream(7)) == stream(7));
    CHECK(slot[0] >= 0 && slot[2] == slot[0]); /* the same thread: the same stream */
    CHECK(slot[1] >= 0 && slot[1] != slot[0]); /* another thread's hipStreamPerThread is another stream */
    CHECK(head[0] == -1 && head[1] == 0);
    /* ... and for a head: a second thread must WAIT for one of the first thread's, it is not the same stream */
    std::atomic<int> got{-1};
    std::thread t3([&] {
        CounterLease h;
        if (h.get(&cc, hipStreamPerThread) == 0) got = h.idx;
    });
    CHECK(wait_until([] { return g_in_wait == 1; }));
    CHECK(got == -1);
    complete_all(cc.slot, MZ_NUM_COUNTERS);
    t3.join();
    CHECK(got >= 0);
    step = 2;
    t1.join();
}

static void held_slots() { // 6
    static ScratchCache c;
    static CounterCache cc;
    static uint32_t words[2 * MZ_NUM_COUNTERS];
    cc.words = words;
    {
        ScratchLease l[kScratchSlots];
        bool seen[kScratchSlots] = {};
        for (int i = 0; i < kScratchSlots; i++) {
            CHECK(l[i].get(&c, 1000, stream(i % 3)) == 0 && !seen[l[i].slot]); /* same stream or not, completed or not: a held slot is nobody else's */
            seen[l[i].slot] = true;
            if (i % 5 == 0) {
                (void)l[i].release();
                CHECK(l[i].get(&c, 1000, stream(i % 3)) == 0);
            }
        }
        ScratchLease one_more;
        CHECK(one_more.get(&c, 1000, stream(0)) == -104 && one_more.slot < 0);
        CHECK(strcmp(g_err, "scratch: more than 32 concurrent launches") == 0);
    }
    {
        CounterLease h[MZ_NUM_COUNTERS];
        bool seen[MZ_NUM_COUNTERS] = {};
        for (int i = 0; i < MZ_NUM_COUNTERS; i++) {
            CHECK(h[i].get(&cc, stream(i % 3)) == 0 && !seen[h[i].idx]);
            seen[h[i].idx] = true;
        }
        CounterLease one_more;
        CHECK(one_more.get(&cc, stream(0)) == -104 && one_more.idx < 0);
        CHECK(strcmp(g_err, "more than 64 launches being set up at once") == 0);
    }
    ScratchLease after;
    CHECK(after.get(&c, 1000, stream(0)) == 0); /* (all given back by the destructors) */
}

// 7: every slot busy on a stream of its own; a launch on one more stream waits for a slot's event -- outside the lock, so a
// second thread takes and gives back a lease (on a stream that has a slot: no wait of its own) meanwhile
template <class Cache, class Lease, class Get>
static void wait_outside_lock(Cache &c, int nslots, Get get, int Lease::*index) {
    for (int i = 0; i < nslots; i++) {
        Lease l;
        CHECK(get(l, stream(i)) == 0 && l.*index == i);
    }
    std::atomic<int> a_slot{-1}, b_slot{-1};
    std::thread a([&] {
        Lease l;
        if (get(l, stream(100)) == 0) a_slot = l.*index;
    });
    CHECK(wait_until([] { return g_in_wait == 1; }));
    std::thread b([&] {
        Lease l;
        if (get(l, stream(5)) == 0) b_slot = l.*index;
    });
    const bool b_done = wait_until([&] { return b_slot >= 0; });
    CHECK(b_done); /* (false: the wait is still under the lock) */
    CHECK(b_slot == 5 && a_slot == -1);
    complete_all(c.slot, nslots);
    a.join();
    b.join();
    CHECK(a_slot >= 0 && a_slot != 5);
    CHECK(!c.slot[a_slot].held && c.slot[a_slot].ev->on == stream(100));
}

static int32_t early_return(ScratchCache *c, CounterCache *cc, hipStream_t s, int *slot, int *head) {
    ScratchLease l;
    int32_t rc = l.get(c, 1000, s);
    if (rc) return rc;
    CounterLease h;
    rc = h.get(cc, s);
    if (rc) return rc;
    *slot = l.slot;
    *head = h.idx;
    if (l.p) return -7; /* (a launcher's error path: no explicit release) */
    return l.release();
}
static void dropped_lease() { // 8
    static ScratchCache c;
    static CounterCache cc;
    static uint32_t words[2 * MZ_NUM_COUNTERS];
    cc.words = words;
    int slot = -1, head = -1;
    CHECK(early_return(&c, &cc, stream(4), &slot, &head) == -7 && slot >= 0 && head >= 0);
    for (const Slot *e : {&c.slot[slot], &cc.slot[head]}) {
        CHECK(!e->held && e->used && e->last == stream(4));
        CHECK(e->ev && e->ev->records == 1 && e->ev->on == stream(4) && !e->ev->done);
    }
    int slot2 = -1, head2 = -1;
    CHECK(early_return(&c, &cc, stream(4), &slot2, &head2) == -7 && slot2 == slot); /* reusable at once on its stream ... */
    ScratchLease other;
    CHECK(other.get(&c, 1000, stream(5)) == 0 && other.slot != slot); /* ... and guarded by its event on any other */
    complete(c.slot[slot].ev);
    ScratchLease third;
    CHECK(third.get(&c, 1000, stream(6)) == 0 && third.slot == slot);
}

static void counter_slots() { // 9 (and 1, 2 for the heads)
    static CounterCache cc;
    static uint32_t words[2 * MZ_NUM_COUNTERS];
    cc.words = words;
    memset(words, 0xFF, sizeof(words));
    for (int round = 0; round < 2; round++)
        for (int i = 0; i < MZ_NUM_COUNTERS; i++) { /* the search starts behind the head handed out last, and wraps */
            CounterLease h;
            CHECK(h.get(&cc, stream(i)) == 0 && h.idx == i && h.p == words + 2 * i);
            CHECK(g_last_memset.p == h.p && g_last_memset.n == 8 && g_last_memset.s == stream(i));
            CHECK(words[2 * i] == 0 && words[2 * i + 1] == 0);
            if (round == 0 && i + 1 < MZ_NUM_COUNTERS) CHECK(words[2 * i + 2] == 0xFFFFFFFFu); /* two words, no more */
            words[2 * i] = words[2 * i + 1] = 77;
        }
    /* every head busy on a stream of its own, none completed: stream 9 gets its own again (stream order), whatever `next` is */
    {
        CounterLease h;
        CHECK(h.get(&cc, stream(9)) == 0 && h.idx == 9 && g_in_wait == 0);
    }
    complete(cc.slot[20].ev); /* another stream gets the one whose launch is over */
    CounterLease h;
    CHECK(h.get(&cc, stream(200)) == 0 && h.idx == 20 && g_in_wait == 0);
}

int main() {
    same_and_other_stream();
    best_fit();
    replace_small_idle();
    stream_per_thread();
    held_slots();
    {
        static ScratchCache c;
        wait_outside_lock<ScratchCache, ScratchLease>(c, kScratchSlots, [&](ScratchLease &l, hipStream_t s) { return l.get(&c, 1000, s); }, &ScratchLease::slot);
        static CounterCache cc;
        static uint32_t words[2 * MZ_NUM_COUNTERS];
        cc.words = words;
        wait_outside_lock<CounterCache, CounterLease>(cc, MZ_NUM_COUNTERS, [&](CounterLease &l, hipStream_t s) { return l.get(&cc, s); }, &CounterLease::idx);
    }
    dropped_lease();
    counter_slots();
    printf("slot cache: %d of %d checks failed\n", g_failed, g_checks);
    return g_failed ? 1 : 0;
}
