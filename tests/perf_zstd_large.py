"""GPU probe (not a pytest): ONE large Zstandard entry decoded three ways -- mzhip_zstd_large (a wave per block),
mzhip_zstd_batch with n = 1 on the same entry (one wave: the kernel the large path falls back to), ZSTD_decompress on one
host thread where libzstd loads.  The entry is text of the benchmark corpus of tests/synth.py (entry() says how), compressed
by libzstd at level 3 where it loads, otherwise by the project's encoder.  The call is made once to allocate its scratch,
then timed once.
Usage: python tests/perf_zstd_large.py [MiB ...]     -- default 8 64 1024; "MiB:skip1" leaves the one-wave run out.
The time per pass (scan, count, emit, resolve, XXH64, CRC) and the pointer-jump rounds are the library's own trace line on
stderr (MZHIP_PAR_TRACE=1, set here)."""
import ctypes as C
import os
import sys
import time
import zlib

os.environ["MZHIP_PAR_TRACE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import gpu_util, synth, zstd_frames as zf  # noqa: E402

mz = gpu_util.mz
L = mz.lib()


_pieces = []


def entry(size):
    """the corpus's words in a random order, as tests/perf_zstd.py makes its 1 MiB entries (the corpus itself is a few MiB:
    repeated as it is, an entry would be one long match).  Up to 64 pieces of 1 MiB are drawn; larger entries repeat those
    64 MiB, further apart than the window of level 3."""
    words = synth.bench_corpus()[0].split()
    rnd = np.random.RandomState(3 + len(_pieces))
    while len(_pieces) < min(64, (size + (1 << 20) - 1) >> 20):
        _pieces.append(b" ".join(words[i] for i in rnd.randint(0, len(words), size=240000))[:1 << 20])
    part = b"".join(_pieces[:min(64, (size + (1 << 20) - 1) >> 20)])
    d = (part * (size // len(part) + 1))[:size]
    if zf.LIBZSTD is not None:
        return d, zf.compress(d, 3, checksum=True), "libzstd level 3"
    st, z, _ = mz.zstd_encode_host(d, 3, True)
    assert st == 0
    return d, z, "the project's encoder, level 3"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def probe(mib, one_wave=True):
    size = mib << 20
    d, z, how = entry(size)
    want = zlib.crc32(d)
    print("entry of %d MiB (%s): %d B compressed, ratio %.3f, checksum on" % (mib, how, len(z), len(z) / size), flush=True)
    d_in = torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    mz.zstd_large(d_in, d_out)      # the first call allocates the scratch
    d_out.zero_()
    print("  -- the timed call:", flush=True)
    ms, (st, ol, iu, crc, s) = wall(lambda: mz.zstd_large(d_in, d_out))
    ok = (st, ol, iu, crc) == (0, size, len(z), want) and s["fallback"] == 0
    print("  mzhip_zstd_large: %.1f ms  %.3f GiB/s out  %s  ok=%s" % (ms, size / 2**30 / (ms / 1e3), s, ok), flush=True)
    if one_wave:
        zero = torch.zeros(1, dtype=torch.int64, device="cuda")
        ln, cap = torch.tensor([len(z)], dtype=torch.int32, device="cuda"), torch.tensor([size], dtype=torch.int32, device="cuda")
        d_out.zero_()
        ms1, r = wall(lambda: mz.zstd_batch(d_in, zero, ln, d_out, zero, cap))
        ok1 = int(r[3].cpu()[0]) == 0 and int(mz.u32(r[2])[0]) == want
        print("  mzhip_zstd_batch, n = 1: %.1f ms  %.4f GiB/s out  ok=%s  -> the wave-per-block call is %.1f x" % (
            ms1, size / 2**30 / (ms1 / 1e3), ok1, ms1 / ms), flush=True)
    if zf.LIBZSTD is not None:
        t0 = time.perf_counter()
        verdict = zf.judge(z, size)[0]
        hs = time.perf_counter() - t0
        print("  ZSTD_decompress, one host thread: %.1f ms  %.3f GiB/s out  %s" % (hs * 1e3, size / 2**30 / hs, verdict), flush=True)


for arg in (sys.argv[1:] or ["8", "64", "1024"]):
    mib, _, opt = arg.partition(":")
    probe(int(mib), one_wave=opt != "skip1")
