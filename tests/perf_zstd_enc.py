"""GPU probe (not a pytest): throughput of the Zstandard batch encode (mzhip_zstd_encode_batch, ZIP method 93) on
device-resident entries of tests/synth.py's corpus, beside ZSTD_compress2 (libzstd, where it loads) on one host thread, and the
output size against libzstd's at the same level.
Usage: python tests/perf_zstd_enc.py [64k|1m|all] [levels, default 1,3]     -- 16 384 x 64 KiB entries and 2 048 x 1 MiB
entries, ONE timed launch each (a launch of one-byte entries with the same geometry comes first: it allocates the scratch).
With a library built by `make PROF=1` (MZHIP_LIB names it) the coding kernel's stage shares are printed too."""
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import gpu_util, synth  # noqa: E402
from tests import zstd_frames as zf  # noqa: E402

mz = gpu_util.mz
L = mz.lib()
which = sys.argv[1] if len(sys.argv) > 1 else "all"
levels = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,3").split(",")]
STAGES = ("sequence build, repeat offsets", "histograms and tables", "literal coding", "sequence coding", "framing, copies, XXH64, CRC-32")


def prof_read(reset):
    if not hasattr(L, "mzhip_prof_read"):
        return None
    buf = (C.c_ulonglong * 32)()
    return list(buf) if L.mzhip_prof_read(buf, reset) == 0 else None


def launch(b, n, size, level, res):
    rc = L.mzhip_zstd_encode_batch(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), size, b["d_out"].data_ptr(),
                                   b["out_off"].data_ptr(), b["out_cap"].data_ptr(), n, level, 0, res[0].data_ptr(), res[1].data_ptr(),
                                   res[2].data_ptr(), None)
    assert rc == 0, (rc, L.mzhip_last_error())


def probe(tag, datas, n_total, level):
    size = len(datas[0])
    host_s, theirs = None, None
    if zf.LIBZSTD is not None:
        t0 = time.perf_counter()
        ref = [zf.compress(d, level) for d in datas]
        host_s = (time.perf_counter() - t0) * n_total / len(datas)   # the unique entries timed, scaled to the batch
        theirs = sum(len(z) for z in ref)
    idx = np.arange(n_total) % len(datas)
    cap = int(L.mzhip_zstd_encode_bound(size))
    b = gpu_util.make_batch([datas[i] for i in idx], [cap] * n_total)
    res = [torch.empty(n_total, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    g, sb = C.c_uint32(0), C.c_uint64(0)
    L.mzhip_zstd_encode_launch_geometry(n_total, size, level, C.byref(g), C.byref(sb))
    one = torch.ones(n_total, dtype=torch.int32, device="cuda:0")
    saved, b["in_len"] = b["in_len"], one
    launch(b, n_total, size, level, res)   # one byte per entry: the scratch of the real launch is allocated here
    torch.cuda.synchronize()
    b["in_len"] = saved
    prof_read(1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch(b, n_total, size, level, res)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    prof = prof_read(1)
    out_len, crc, status = res[0].cpu().numpy().astype(np.int64), mz.u32(res[1]), res[2].cpu().numpy()
    want = np.array([zlib.crc32(d) for d in datas], dtype=np.uint32)[idx]
    ok = bool((status == 0).all() and (crc == want).all())
    h_out = b["d_out"].cpu().numpy()
    for i in range(len(datas)):   # the unique entries, read back by the plain reader (64 KiB) or libzstd
        o = int(b["h_out_off"][i])
        z = h_out[o:o + int(out_len[i])].tobytes()
        if zf.LIBZSTD is not None:
            ok = ok and zf.judge(z, size) == ("valid", datas[i])
        elif size <= 65536:
            ok = ok and zf.expand(z) == (0, datas[i], len(z))
    mine = int(out_len[:len(datas)].sum())
    print("zstd encode (%s, level %d): %d x %d B, grid %d waves, scratch %.2f GiB: %.1f ms  %.3f GiB/s in  ok=%s" % (
        tag, level, n_total, size, g.value, sb.value / 2**30, ms, n_total * size / 2**30 / (ms / 1e3), ok), flush=True)
    if theirs is not None:
        print("  output %d bytes for the %d unique entries, libzstd level %d %d: %+.2f %%; ratio %.3f" % (
            mine, len(datas), level, theirs, 100.0 * (mine - theirs) / theirs, mine / (len(datas) * size)), flush=True)
        print("  ZSTD_compress2 of the same entries, one host thread (%d unique timed, scaled): %.1f s  %.3f GiB/s" % (
            len(datas), host_s, n_total * size / 2**30 / host_s), flush=True)
    else:
        print("  output %d bytes for the %d unique entries; ratio %.3f (libzstd does not load here)" % (mine, len(datas), mine / (len(datas) * size)),
              flush=True)
    if prof is not None and sum(prof[27:32]):
        tot = float(sum(prof[27:32]))
        print("  coding kernel, cycles by stage: " + "; ".join("%s %.1f %%" % (s, 100.0 * v / tot) for s, v in zip(STAGES, prof[27:32])), flush=True)


for level in levels:
    if which in ("64k", "all"):
        probe("64 KiB entries", synth.slices(256, 65536, 1234), 16384, level)
    if which in ("1m", "all"):
        rnd = np.random.RandomState(3)
        words = synth.corpus().split()
        probe("1 MiB entries", [b" ".join(words[i] for i in rnd.randint(0, len(words), size=240000))[:1 << 20] for _ in range(8)], 2048, level)
