"""GPU probe (not a pytest): throughput of the Zstandard batch decode (mzhip_zstd_batch, ZIP method 93) on device-resident
entries of tests/synth.py's corpus compressed by libzstd at level 3, beside ZSTD_decompress on one host thread.
Usage: python tests/perf_zstd.py [64k|1m|all]     -- 16 384 x 64 KiB entries, 2 048 x 1 MiB entries.  The project has no
zstd encoder, so the probe needs libzstd for its inputs.
With a measurement build of the library (make PROF=1) the cycle share of the kernel's stages is printed too."""
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import gpu_util, synth, zstd_frames as zf  # noqa: E402

mz = gpu_util.mz
L = mz.lib()
which = sys.argv[1] if len(sys.argv) > 1 else "all"
STAGES = {23: "headers + tables", 24: "literal streams", 25: "sequence decode", 26: "execution (literal and match copies)", 27: "XXH64 + CRC-32"}
if zf.LIBZSTD is None:
    sys.exit("libzstd does not load: no inputs")


def timed(fn, reps=2):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def probe(name, datas, n_total):
    size = len(datas[0])
    pays = [zf.compress(d, 3, checksum=True) for d in datas]
    t0 = time.perf_counter()
    for p in pays:
        zf.judge(p, size)
    host_s = (time.perf_counter() - t0) * n_total / len(pays)   # the unique entries timed, scaled to the batch
    idx = np.arange(n_total) % len(datas)
    b = gpu_util.make_batch([pays[i] for i in idx], [size] * n_total)
    out_len, in_used, crc, status = (torch.empty(n_total, dtype=torch.int32, device="cuda:0") for _ in range(4))
    g, sb = C.c_uint32(0), C.c_uint64(0)
    L.mzhip_zstd_launch_geometry(n_total, C.byref(g), C.byref(sb))

    def run():
        assert L.mzhip_zstd_batch(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), b["d_out"].data_ptr(),
                                  b["out_off"].data_ptr(), b["out_cap"].data_ptr(), n_total, out_len.data_ptr(), in_used.data_ptr(),
                                  crc.data_ptr(), status.data_ptr(), None) == 0
    run()   # the first launch allocates the scratch
    if hasattr(L, "mzhip_prof_read"):
        L.mzhip_prof_read((C.c_ulonglong * 32)(), 1)
    ms = timed(run)
    want = np.array([zlib.crc32(d) for d in datas], dtype=np.uint32)[idx]
    ok = bool((status.cpu().numpy() == 0).all() and (mz.u32(crc) == want).all())
    print("zstd decode (%s): %d x %d B, level 3, ratio %.3f, grid %d waves, scratch %.3f GiB: %.1f ms  %.3f GiB/s out  ok=%s" % (
        name, n_total, size, sum(len(p) for p in pays) / (len(pays) * size), g.value, sb.value / 2**30, ms,
        n_total * size / 2**30 / (ms / 1e3), ok), flush=True)
    print("  ZSTD_decompress of the same entries, one host thread (%d unique timed, scaled): %.1f s  %.3f GiB/s" % (
        len(pays), host_s, n_total * size / 2**30 / host_s), flush=True)
    if hasattr(L, "mzhip_prof_read"):
        buf = (C.c_ulonglong * 32)()
        L.mzhip_prof_read(buf, 1)
        tot = float(sum(buf[i] for i in STAGES)) or 1.0
        for i in sorted(STAGES):
            print("  %-38s %5.1f %%" % (STAGES[i], 100.0 * buf[i] / tot), flush=True)


if which in ("64k", "all"):
    probe("64 KiB entries", synth.slices(256, 65536, 1234), 16384)
if which in ("1m", "all"):
    rnd = np.random.RandomState(3)
    words = synth.corpus().split()
    probe("1 MiB entries", [b" ".join(words[i] for i in rnd.randint(0, len(words), size=240000))[:1 << 20] for _ in range(8)], 2048)
