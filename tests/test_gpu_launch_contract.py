"""The contract include/mzhip.h states once for all batch entry points -- "`stream` is a hipStream_t passed as void* ...
Asynchronous on `stream`", 64-bit offset arrays -- held against every row of tests/launch_cases.py (the 19 batch entry points
and the two synchronous large-entry calls), every comparison exact:

  B1 test_stream_order*        On a non-blocking stream, with nothing but stream order between them: a plug (a device
                               operation of known length), the real payload bytes copied over a decoy, the call, a copy of
                               every result array and of the output, a refill of both with pattern and sentinels.  A kernel
                               or memset queued on another stream reads the decoy (valid streams of the same lengths whose
                               results differ in every entry) or loses its results to the refill.  The second call on the
                               same stream must return while the plug still runs: no call waits for the stream.  The two
                               large-entry calls are synchronous by contract: results, and the upload queued just before.
  B2 test_stream_per_thread    hipStreamPerThread (the handle 2) from four threads, each through every row with its own seed,
                               each synchronising only its own stream.
  B3 test_everything_in_flight*  Behind a gate, 12 streams x 3 rounds = 36 launches queued without a host synchronisation (more
                               than the 32 scratch slots), every launch another row and seed than its neighbours; the same
                               from 4 threads with 3 streams each, the two large-entry calls among them.  Scratch, a retry
                               list or a work-queue head shared by two launches shows as another launch's bytes.
  B4 test_offsets_beyond_4gib* Entries placed in two device tensors of 2^32 + 2^29 bytes so that an entry straddles offset 2^31,
                               offset 2^32, lies wholly above 2^32 (a decoy at offset - 2^32) or straddles a 4 GiB-aligned
                               device address; out_cap 0x80000000 and 0xFFFFFFFF where the room behind the entry allows; every
                               byte of both tensors outside the entries still holds the fill value afterwards.

MEASURED (see the fixture `plug`, which prints them): the time of one launch per row on an idle device, and the plug -- at
least 20 times the longest of them and at least 50 ms.
"""
import ctypes as C
import statistics
import threading
import time

import numpy as np
import pytest

from tests import launch_cases as lc

pytestmark = pytest.mark.gpu
SENT = int(np.array([0x5EED5EED], dtype=np.uint32).view(np.int32)[0])
TIMES = {}
LARGE_SEED = 3        # one seed for the two large entries everywhere: their host reference takes seconds per MiB


@pytest.fixture(scope="module")
def gpu():
    import torch

    from tests import gpu_util

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    t0 = time.time()
    yield gpu_util
    print("\nlaunch contract: wall time per test %s; module %.1f s" % (", ".join("%s %.2f s" % kv for kv in TIMES.items()), time.time() - t0))


@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.time()
    yield
    TIMES[request.node.name] = time.time() - t0


# ---- a launch of one row: buffers, call, check ----------------------------------------------------------------------------

def prepare(gpu, row, seed, upload="real", fill=None):
    """buffers of one launch of a row: the layout of gpu_util.make_batch with red zones and odd offsets over a seeded pattern,
    guarded result arrays, the row's other arrays on the device.  upload: "real" or "decoy" payload bytes in d_in."""
    import torch

    pays, caps, extra = row.build(seed)
    b = gpu.make_batch(pays, [0] * len(pays) if row.kind == "sum" else caps, guard=lc.GUARD, fill=(seed % 1000 + 1) if fill is None else fill,
                       align=1, odd=True, upload_payloads=upload == "real")
    return _finish(gpu, row, seed, b, pays, caps, extra, upload)


def _finish(gpu, row, seed, b, pays, caps, extra, upload="real"):
    import torch

    if upload == "decoy":
        b["d_in"].copy_(torch.from_numpy(gpu.payload_blob(b, row.decoy(seed))))
    if extra.get("prefix"):                       # the history in front of a resumed stream's room is the caller's
        for i, h in enumerate(extra["prefix"]):
            o = int(b["h_out_off"][i])
            b["h_fill"][o:o + len(h)] = np.frombuffer(h, dtype=np.uint8)
        b["d_out"].copy_(torch.from_numpy(b["h_fill"]))
    b["x"] = {k: torch.from_numpy(v).to(b["in_off"].device) for k, v in extra.get("dev", {}).items()}
    b["extra"] = extra
    names, words = row.results(extra)
    return dict(row=row, seed=seed, b=b, R=gpu.guarded_results(b["n"], names, words=words), words=words, extra=extra,
                exp=row.expect(pays, caps, extra))


def check(gpu, job, R=None, d_out=None, where=()):
    """a finished launch against expect(), then the guards: nothing outside the regions, the input unchanged, result elements
    behind n untouched, a status-0 entry's bytes behind out_len untouched"""
    row, b, exp = job["row"], dict(job["b"]), job["exp"]
    n = b["n"]
    R = job["R"] if R is None else R
    if d_out is not None:
        b["d_out"] = d_out
    w = {k: gpu.result_words(R[k], n, job["words"].get(k, 1)) for k in R}
    h = b["d_out"].detach().cpu().numpy()
    off, cap = b["h_out_off"], b["h_out_cap"]
    lc.verify(row, exp, job["extra"], w, lambda i: h[int(off[i]):int(off[i]) + int(cap[i])].tobytes(), where)
    status = np.array([e["words"].get("status", 0) for e in exp], dtype=np.uint32).view(np.int32)
    out_len = w["out_len"].astype(np.int64) if "out_len" in w else np.zeros(n, dtype=np.int64)
    gpu.check_guards(b, out_len, status, results=R, words=job["words"], slack_ok=any(e.get("clamped") for e in exp), outputs=row.kind != "sum")
    for i, e in enumerate(exp):                 # the crypt calls write [out_off, out_off + out_len) and not a byte more, whatever the status
        if e.get("exact_region"):
            lo, hi = int(off[i]) + int(out_len[i]), int(off[i]) + int(cap[i])
            assert (h[lo:hi] == b["h_fill"][lo:hi]).all(), (where, row.name, i, "bytes behind out_len written")


class LargeJob:
    """one large entry between red zones of pattern, the decoy in d_in until the real bytes are copied over it"""

    G = 4096

    def __init__(self, gpu, row, seed, upload="real"):
        import torch

        G = self.G
        self.row, self.gpu = row, gpu
        self.z, self.cap = row.build(seed)
        self.exp = row.expect(self.z, self.cap)
        self.h_in = gpu.guard_pattern(G + len(self.z) + G, 71)
        self.h_in[G:G + len(self.z)] = np.frombuffer(self.z, dtype=np.uint8)
        first = self.h_in.copy()
        if upload == "decoy":
            first[G:G + len(self.z)] = np.frombuffer(row.decoy(seed), dtype=np.uint8)
        self.d_in = torch.from_numpy(first).cuda()
        self.h_fill = gpu.guard_pattern(G + self.cap + G, 72)
        self.d_out = torch.from_numpy(self.h_fill.copy()).cuda()
        self.res = [C.c_uint32(0x5EED5EED) for _ in range(3)] + [C.c_int32(0x5EED)]

    def call(self, stream):
        return self.row.call(self.gpu.mz.lib(), self.d_in.data_ptr() + self.G, len(self.z), self.d_out.data_ptr() + self.G, self.cap, self.res, stream)

    def check(self, where=()):
        G, e = self.G, self.exp
        got = dict(out_len=self.res[0].value, in_used=self.res[1].value, crc=self.res[2].value, status=self.res[3].value & 0xFFFFFFFF)
        assert got == e["words"], (where, self.row.name, got, e["words"])
        h = self.d_out.cpu().numpy()
        n = len(e["out"])
        assert h[G:G + n].tobytes() == e["out"], (where, self.row.name, "bytes")
        h[G:G + n] = self.h_fill[G:G + n]
        bad = np.flatnonzero(h != self.h_fill)
        assert bad.size == 0, (where, self.row.name, "byte %d of the output buffer (%d in the entry's room of %d, out_len %d) was written" % (int(bad[0]), int(bad[0]) - G, self.cap, n))
        assert (self.d_in.cpu().numpy() == self.h_in).all(), (where, self.row.name, "input changed")


# ---- the plug -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plug(gpu):
    """{"fn": queues the plug on torch's current stream, "ms": its measured length, "launch_ms": {row: one launch on an idle
    device, the median of three after a first}}.  The plug is torch.cuda._sleep with its cycle count calibrated against event
    timing here; where that gives nothing usable, a chain of fills of a 1 GiB tensor."""
    import torch

    L = gpu.mz.lib()
    launch_ms = {}
    for row in lc.ROWS:
        job = prepare(gpu, row, 1)
        torch.cuda.synchronize()
        ts = []
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert row.call(L, job["b"], job["R"], None) == 0, L.mzhip_last_error()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        launch_ms[row.name] = statistics.median(ts[1:])
    for row in lc.LARGE:
        job = LargeJob(gpu, row, LARGE_SEED)
        torch.cuda.synchronize()
        ts = []
        for _ in range(4):
            t0 = time.perf_counter()
            assert job.call(None) == 0, L.mzhip_last_error()
            ts.append((time.perf_counter() - t0) * 1e3)
        launch_ms[row.name] = statistics.median(ts[1:])
    want = max(50.0, 20.0 * max(launch_ms.values()))
    assert want < 3000.0, launch_ms                                   # (a launch of 8 small entries that takes 150 ms is a finding of its own)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    fn = None
    if hasattr(torch.cuda, "_sleep"):
        probe = 20000000
        timed(lambda: torch.cuda._sleep(probe))
        per = statistics.median(timed(lambda: torch.cuda._sleep(probe)) for _ in range(3)) / probe
        if per * probe > 1.0:                                       # the spin kernel really spins: at least a millisecond for the probe
            cycles = int(1.25 * want / per)
            fn, how = (lambda: torch.cuda._sleep(cycles)), "torch.cuda._sleep(%d)" % cycles
    if fn is None:
        pad = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
        one = statistics.median(timed(lambda: pad.fill_(1)) for _ in range(4)[1:])
        reps = int(1.25 * want / one) + 1

        def fn():
            for _ in range(reps):
                pad.fill_(1)
        how = "%d fills of 1 GiB" % reps
    ms = statistics.median(timed(fn) for _ in range(3))
    print("\none launch on an idle device, ms: %s; longest %.3f; plug wanted >= %.1f ms, used: %s = %.1f ms"
          % (", ".join("%s %.3f" % (k.replace("mzhip_", ""), v) for k, v in launch_ms.items()), max(launch_ms.values()), want, how, ms))
    assert ms >= want, (ms, want)
    return dict(fn=fn, ms=ms, launch_ms=launch_ms)


# ---- B1: stream order -------------------------------------------------------------------------------------------------------

class NullProbe:
    """Is the null stream free while the plug runs on `s`?  Streams share the few hardware queues of a process, and work on
    the null stream whose queue also serves the plugged stream runs behind the plug: a kernel that escaped there would look
    ordered, and the run would prove nothing.  So every run queues, right behind its plug, a small fill on the null stream
    with an event behind it; the run is SIGHTED when that event is over while the plug still runs.  An escaped kernel sits
    behind the fill on the same stream, so in a sighted run it has read the decoy long before the real bytes arrive."""

    def __init__(self):
        import torch

        self.x = torch.zeros(1024, dtype=torch.int32, device="cuda:0")

    def queue(self):
        import torch

        null = torch.cuda.default_stream()
        with torch.cuda.stream(null):
            self.x.fill_(1)
            self.done = torch.cuda.Event()
            self.done.record(null)

    def sighted(self, s):
        t0 = time.perf_counter()
        while not self.done.query() and time.perf_counter() - t0 < 0.02:
            pass
        return self.done.query() and not s.query()


@pytest.mark.parametrize("row", lc.ROWS, ids=lambda r: r.name)
def test_stream_order(gpu, plug, row):
    import torch

    L = gpu.mz.lib()
    job = prepare(gpu, row, 3, upload="decoy")
    b, R = job["b"], job["R"]
    pin_real = torch.from_numpy(b["h_in"]).pin_memory()
    pin_decoy = torch.from_numpy(gpu.payload_blob(b, row.decoy(3))).pin_memory()
    pin_fill = torch.from_numpy(b["h_fill"]).pin_memory()
    probe = NullProbe()
    sighted = []
    for attempt in range(4):                                      # another stream until both runs on one are sighted
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        takes = []
        with torch.cuda.stream(s):                                # from here on nothing but stream order
            for run in range(2):
                b["d_in"].copy_(pin_decoy, non_blocking=True)
                plug["fn"]()
                probe.queue()
                b["d_in"].copy_(pin_real, non_blocking=True)
                rc = row.call(L, b, R, s.cuda_stream)
                busy = not s.query()
                assert rc == 0, (rc, L.mzhip_last_error())
                takes.append(({k: t.clone() for k, t in R.items()}, b["d_out"].clone(), busy, probe.sighted(s)))
                b["d_out"].copy_(pin_fill, non_blocking=True)
                for t in R.values():
                    t.fill_(SENT)
        s.synchronize()
        torch.cuda.synchronize()
        for run, (Rc, oc, _, _) in enumerate(takes):
            check(gpu, job, Rc, oc, ("attempt", attempt, "run", run))
        assert takes[1][2], "%s waited for the stream: the plug (%.0f ms) had run out when the second call returned" % (row.name, plug["ms"])
        assert (b["d_out"].cpu().numpy() == b["h_fill"]).all(), "a store landed behind the refill: not ordered on the stream"
        for k, t in R.items():
            assert (t.cpu().numpy() == SENT).all(), (k, "a result landed behind the refill: not ordered on the stream")
        sighted.append([t[3] for t in takes])
        if all(sighted[-1]):
            break
    assert all(sighted[-1]), "on none of 4 streams was the null stream free during the plug: %s" % sighted


@pytest.mark.parametrize("row", lc.LARGE, ids=lambda r: r.name)
def test_stream_order_large(gpu, plug, row):
    """synchronous by contract: the call returns with the results; the upload queued on the stream just before it (behind a plug)
    is what it decodes"""
    import torch

    job = LargeJob(gpu, row, LARGE_SEED, upload="decoy")
    pin_real = torch.from_numpy(job.h_in).pin_memory()
    probe = NullProbe()
    pin_decoy = torch.from_numpy(np.frombuffer(row.decoy(LARGE_SEED), dtype=np.uint8).copy()).pin_memory()
    sighted = []
    for attempt in range(4):
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            job.d_in[job.G:job.G + len(job.z)].copy_(pin_decoy, non_blocking=True)
            plug["fn"]()
            probe.queue()
            job.d_in.copy_(pin_real, non_blocking=True)
            sighted.append(probe.sighted(s))                      # (the call below returns when the stream is through)
            rc = job.call(s.cuda_stream)
        assert rc == 0, (rc, gpu.mz.lib().mzhip_last_error())
        job.check(("large", attempt))
        torch.cuda.synchronize()
        if sighted[-1]:
            break
        job.d_out.copy_(torch.from_numpy(job.h_fill))
    assert sighted[-1], "on none of 4 streams was the null stream free during the plug: %s" % sighted


# ---- B2: hipStreamPerThread ----------------------------------------------------------------------------------------------

def _hip_runtime():
    """the HIP runtime libmzhip.so has loaded (the one already mapped into this process)"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                lib = C.CDLL(line.split()[-1])
                lib.hipStreamSynchronize.restype = C.c_int
                lib.hipStreamSynchronize.argtypes = [C.c_void_p]
                return lib
    raise AssertionError("no HIP runtime mapped")


def _threads(fn, n):
    errors = []

    def run(t):
        try:
            fn(t)
        except BaseException as e:                                   # noqa: BLE001 - reported below
            import traceback

            errors.append((t, repr(e), traceback.format_exc()[-1500:]))

    ths = [threading.Thread(target=run, args=(t,)) for t in range(n)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors


def test_stream_per_thread(gpu):
    import torch

    L = gpu.mz.lib()
    hip = _hip_runtime()
    PER_THREAD = C.c_void_p(2)
    jobs = {t: [prepare(gpu, row, 20 + t) for row in lc.ROWS] for t in range(4)}
    torch.cuda.synchronize()
    start = threading.Barrier(4)

    def worker(t):
        torch.cuda.set_device(0)
        start.wait()
        for job in jobs[t]:
            rc = job["row"].call(L, job["b"], job["R"], PER_THREAD)
            assert rc == 0, (t, job["row"].name, rc, L.mzhip_last_error())
        assert hip.hipStreamSynchronize(PER_THREAD) == 0                # this thread's stream and no other
        for job in jobs[t]:
            check(gpu, job, where=("thread", t))

    _threads(worker, 4)


# ---- B3: everything in flight together ------------------------------------------------------------------------------------

def _row_of(k, r):
    return lc.ROWS[(k + 12 * r) % len(lc.ROWS)]


def test_everything_in_flight(gpu, plug):
    import torch

    L = gpu.mz.lib()
    assert sorted(set(_row_of(k, r).name for r in range(3) for k in range(12))) == sorted(r.name for r in lc.ROWS)
    jobs = [[prepare(gpu, _row_of(k, r), 100 + 12 * r + k) for k in range(12)] for r in range(3)]
    gate, streams = torch.cuda.Stream(), [torch.cuda.Stream() for _ in range(12)]
    opened = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(gate):
        plug["fn"]()
        opened.record()
    for s in streams:
        s.wait_event(opened)
    for r in range(3):
        for k, s in enumerate(streams):
            rc = jobs[r][k]["row"].call(L, jobs[r][k]["b"], jobs[r][k]["R"], s.cuda_stream)
            assert rc == 0, (r, k, rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    for r in range(3):
        for k in range(12):
            check(gpu, jobs[r][k], where=("round", r, "stream", k))


def test_everything_in_flight_from_threads(gpu, plug):
    import torch

    L = gpu.mz.lib()
    jobs = [[prepare(gpu, _row_of(k, r + 1), 200 + 12 * r + k) for k in range(12)] for r in range(3)]
    large = [LargeJob(gpu, row, LARGE_SEED) for row in lc.LARGE]
    gate, streams = torch.cuda.Stream(), [torch.cuda.Stream() for _ in range(12)]
    opened = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(gate):
        plug["fn"]()
        opened.record()
    for s in streams:
        s.wait_event(opened)
    start = threading.Barrier(4)

    def worker(t):
        torch.cuda.set_device(0)
        start.wait()
        for r in range(3):
            for k in range(3 * t, 3 * t + 3):
                rc = jobs[r][k]["row"].call(L, jobs[r][k]["b"], jobs[r][k]["R"], streams[k].cuda_stream)
                assert rc == 0, (t, r, k, rc, L.mzhip_last_error())
        if t < 2:             # synchronous: returns when the gate has opened and its passes, each with leases of its own, are through
            rc = large[t].call(streams[3 * t].cuda_stream)
            assert rc == 0, (t, "large", rc, L.mzhip_last_error())

    _threads(worker, 4)
    torch.cuda.synchronize()
    for r in range(3):
        for k in range(12):
            check(gpu, jobs[r][k], where=("round", r, "stream", k))
    for j in large:
        j.check("threads")


# ---- B4: offsets at and above 2^31 and 2^32 ----------------------------------------------------------------------------------

BIG = (1 << 32) + (1 << 29)
FILL = 0xA5


@pytest.fixture(scope="module")
def big(gpu):
    """one input and one output tensor of 2^32 + 2^29 bytes, every byte FILL"""
    import torch

    try:
        t_in = torch.empty(BIG, dtype=torch.uint8, device="cuda:0")
        t_out = torch.empty(BIG, dtype=torch.uint8, device="cuda:0")
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip("no device memory for two tensors of 2^32 + 2^29 bytes: %s" % str(e)[:200])
    t_in.fill_(FILL)
    t_out.fill_(FILL)
    torch.cuda.synchronize()
    yield t_in, t_out
    del t_in, t_out
    torch.cuda.empty_cache()


def _all_fill(t, what):
    """every byte of the tensor holds FILL: compared on the device, 256 MiB at a time"""
    import torch

    v = t.view(torch.int64)
    want = int.from_bytes(bytes([FILL]) * 8, "little", signed=True)
    step = 1 << 25
    for o in range(0, v.numel(), step):
        c = v[o:o + step]
        if not bool((c == want).all()):
            j = 8 * (o + int(torch.nonzero(c != want)[0]))
            k = j + int(np.flatnonzero(t[j:j + 8].cpu().numpy() != FILL)[0])
            raise AssertionError("%s: byte at offset %d (0x%x) of the tensor, outside every entry, was written: %d" % (what, k, k, int(t[k])))


ABOVE_IN, ABOVE_OUT = (1 << 32) + (3 << 20) + 5, (1 << 32) + (5 << 20) + 7     # where the entries wholly above 2^32 start


def _boundaries(t):
    """offsets inside the tensor an entry is made to straddle: 2^31, 2^32, none (the place wholly above 2^32), and the first
    4 GiB-aligned DEVICE ADDRESS at least 2^28 bytes inside -- where that lies within 16 MiB of one of the other places (an
    allocation aligned to 2^31 or more: the address is straddled there already), 3 * 2^30 instead"""
    a = t.data_ptr()
    d = ((a + (1 << 28) + (1 << 32) - 1) >> 32 << 32) - a
    assert (1 << 28) <= d < (1 << 28) + (1 << 32) and (a + d) % (1 << 32) == 0
    if min(abs(d - x) for x in (1 << 31, 1 << 32, ABOVE_IN, ABOVE_OUT)) < (1 << 24):
        d = 3 << 30
    return [1 << 31, 1 << 32, None, d]


@pytest.mark.parametrize("row", lc.ROWS, ids=lambda r: r.name)
def test_offsets_beyond_4gib(gpu, big, row):
    import torch

    t_in, t_out = big
    L = gpu.mz.lib()
    seed = 4
    pays, caps, extra = row.build(seed)
    dec = row.decoy(seed)
    region = [0] * lc.N if row.kind == "sum" else caps
    G = lc.GUARD
    subs = []
    for k, (bi, bo) in enumerate(zip(_boundaries(t_in), _boundaries(t_out))):
        e = (2 * k, 2 * k + 1)
        # (make_batch, guard G, align 1, odd: the first entry's input starts at G, its output at G | 1)
        in_base = ABOVE_IN if bi is None else bi - G - len(pays[e[0]]) // 2
        out_base = ABOVE_OUT if bo is None else bo - (G | 1) - region[e[0]] // 2
        sb = gpu.make_batch([pays[i] for i in e], [region[i] for i in e], guard=G, fill=40 + k, align=1, odd=True,
                            into=(t_in, in_base, t_out, out_base))
        if bi is None:          # what an offset narrowed to 32 bits would read: the decoy's entries, 2^32 bytes below
            lo = in_base - (1 << 32)
            sb["alias"] = t_in[lo:lo + sb["h_in"].size]
            sb["alias"].copy_(torch.from_numpy(gpu.payload_blob(sb, [dec[i] for i in e])))
        else:
            o, n = int(sb["h_in_off"][0]) + in_base, len(pays[e[0]])
            assert o < bi < o + n, "entry %d's input does not straddle offset 0x%x" % (e[0], bi)
        subs.append(sb)
    b = dict(n=lc.N, p_in=t_in.data_ptr(), p_out=t_out.data_ptr())
    for key in ("in_off", "in_len", "out_off", "out_cap"):
        b[key] = torch.cat([sb[key] for sb in subs]).contiguous()
    h_off = b["out_off"].cpu().numpy()
    dev_caps = list(caps)
    if row.kind == "codec" and not row.cap_tied:      # the streams are short: nothing near these caps is written
        cap32 = np.array(region, dtype=np.int64)
        for i, giant in ((1, 0x80000000), (6, 0xFFFFFFFF)):
            if int(h_off[i]) + giant <= BIG:
                cap32[i] = dev_caps[i] = giant
        assert dev_caps[1] == 0x80000000
        b["out_cap"] = torch.from_numpy(cap32.astype(np.uint32).view(np.int32)).to(t_in.device)
    b["x"] = {k: torch.from_numpy(v).to(t_in.device) for k, v in extra.get("dev", {}).items()}
    b["extra"] = extra
    for k, sb in enumerate(subs):
        for j, i in enumerate((2 * k, 2 * k + 1)):
            h = extra.get("prefix", [b""] * lc.N)[i]
            o = int(sb["h_out_off"][j])
            sb["h_fill"][o:o + len(h)] = np.frombuffer(h, dtype=np.uint8)
        sb["d_out"].copy_(torch.from_numpy(sb["h_fill"]))
    names, words = row.results(extra)
    R = gpu.guarded_results(lc.N, names, words=words)
    exp = row.expect(pays, dev_caps, extra)
    torch.cuda.synchronize()
    rc = row.call(L, b, R, None)
    assert rc == 0, (rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    w = {k: gpu.result_words(R[k], lc.N, words.get(k, 1)) for k in R}
    hs = [sb["d_out"].cpu().numpy().copy() for sb in subs]
    for sb, h in zip(subs, hs):                       # host copies of the places, then the places themselves back to FILL:
        keep = torch.from_numpy(h), sb["d_in"].cpu().clone()  # not a byte of either tensor may differ from it now
        sb["d_in"].fill_(FILL)
        sb["d_out"].fill_(FILL)
        if "alias" in sb:
            sb["alias"].fill_(FILL)
        sb["d_out"], sb["d_in"] = keep
    _all_fill(t_out, "%s, output tensor" % row.name)
    _all_fill(t_in, "%s, input tensor" % row.name)

    def region_of(i):
        sb, j = subs[i // 2], i % 2
        o = int(sb["h_out_off"][j])
        return hs[i // 2][o:o + int(sb["h_out_cap"][j])].tobytes()

    lc.verify(row, exp, extra, w, region_of, "beyond 4 GiB")
    for name, t in R.items():
        a = t.cpu().numpy().view(np.uint32)
        assert (a[lc.N * words.get(name, 1):] == 0x5EED5EED).all(), (name, "an element behind n was written")
    status = np.array([e["words"].get("status", 0) for e in exp], dtype=np.uint32).view(np.int32)
    out_len = w["out_len"].astype(np.int64) if "out_len" in w else np.zeros(lc.N, dtype=np.int64)
    for k, sb in enumerate(subs):                     # red zones around each placed region, the input unchanged, the slack of status 0
        gpu.check_guards(sb, out_len[2 * k:2 * k + 2], status[2 * k:2 * k + 2], slack_ok=any(e.get("clamped") for e in exp), outputs=row.kind != "sum")
        for j, i in enumerate((2 * k, 2 * k + 1)):
            if exp[i].get("exact_region"):
                lo, hi = int(sb["h_out_off"][j]) + int(out_len[i]), int(sb["h_out_off"][j]) + int(sb["h_out_cap"][j])
                assert (hs[k][lo:hi] == sb["h_fill"][lo:hi]).all(), (row.name, i, "bytes behind out_len written")


@pytest.mark.parametrize("row", lc.LARGE, ids=lambda r: r.name)
def test_offsets_beyond_4gib_large(gpu, big, row):
    """the large entry where its input straddles offset 2^32 and its output offset 2^31, then wholly above 2^32 (the decoy
    2^32 bytes below) with the output across the 4 GiB-aligned device address"""
    import torch

    t_in, t_out = big
    L = gpu.mz.lib()
    z, cap = row.build(LARGE_SEED)
    e = row.expect(z, cap)
    dz = torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy())
    for in_off, out_off, alias in (((1 << 32) - len(z) // 2, (1 << 31) - cap // 3, False),
                                   (ABOVE_IN, _boundaries(t_out)[3] - cap // 2, True)):
        assert in_off + len(z) <= BIG and 0 <= out_off and out_off + cap <= BIG
        t_in[in_off:in_off + len(z)].copy_(dz)
        if alias:
            t_in[in_off - (1 << 32):in_off - (1 << 32) + len(z)].copy_(torch.from_numpy(np.frombuffer(row.decoy(LARGE_SEED), dtype=np.uint8).copy()))
        res = [C.c_uint32(0x5EED5EED) for _ in range(3)] + [C.c_int32(0x5EED)]
        torch.cuda.synchronize()
        rc = row.call(L, t_in.data_ptr() + in_off, len(z), t_out.data_ptr() + out_off, cap, res, None)
        assert rc == 0, (rc, L.mzhip_last_error())
        torch.cuda.synchronize()
        got = dict(out_len=res[0].value, in_used=res[1].value, crc=res[2].value, status=res[3].value & 0xFFFFFFFF)
        assert got == e["words"], (row.name, in_off, got, e["words"])
        n = len(e["out"])
        assert t_out[out_off:out_off + n].cpu().numpy().tobytes() == e["out"], (row.name, in_off, "bytes")
        assert t_in[in_off:in_off + len(z)].cpu().numpy().tobytes() == z, (row.name, "input changed")
        t_out[out_off:out_off + n].fill_(FILL)
        t_in[in_off:in_off + len(z)].fill_(FILL)
        if alias:
            t_in[in_off - (1 << 32):in_off - (1 << 32) + len(z)].fill_(FILL)
        _all_fill(t_out, "%s, output tensor" % row.name)
        _all_fill(t_in, "%s, input tensor" % row.name)
