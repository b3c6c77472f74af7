"""GPU probe (not a pytest): throughput of the four crypt kernels at 65 536 x 64 KiB, device-resident.
Usage: python tests/perf_crypt.py [n_entries]            HIP-event times of the two C ABI calls (and of the AES call with a
                                                          wrong password, where only the key kernel has work)
       python tests/perf_crypt.py --stats kernel_stats.csv [n_entries]
                                                          GiB/s per kernel from the `rocprofv3 --kernel-trace --stats` table
                                                          of a run of the first form (the three AES kernels share one call)
Sixteen distinct entries made by tests/crypt_ref.py are replicated in HBM, so every entry's bytes are read from memory."""
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SIZE, UNIQUE, STRENGTH = 65536, 16, 3
PW = b"test123"
args = [a for a in sys.argv[1:] if a != "--stats"]
stats = args.pop(0) if "--stats" in sys.argv else None
N = int(args[0]) if args else 65536
GIB = N * SIZE / 2**30

if stats:
    with open(stats) as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        avg = float(r.get("AverageNs") or r.get("Average") or 0)
        for k in ("k_pkcrypt_batch", "k_wzaes_keys", "k_wzaes_ctr", "k_wzaes_auth"):
            if name.startswith(k) and avg:
                print("%-16s %4s calls  %9.3f ms average  %8.1f GiB/s of payload" % (k, r.get("Calls", "?"), avg / 1e6, GIB / (avg / 1e9)))
    sys.exit(0)

import torch  # noqa: E402

from tests import crypt_ref as cr  # noqa: E402
from tests import gpu_util  # noqa: E402

L = gpu_util.mz.lib()
dev = torch.device("cuda:0")
rnd = np.random.RandomState(1)


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
    return best


def resident(entries):
    """UNIQUE entries, each in a stride of its length rounded up to 64, replicated to N entries in HBM"""
    stride = (len(entries[0]) + 63) // 64 * 64
    blob = np.zeros(UNIQUE * stride, dtype=np.uint8)
    for i, e in enumerate(entries):
        blob[i * stride:i * stride + len(e)] = np.frombuffer(e, dtype=np.uint8)
    d_in = torch.from_numpy(blob).to(dev).repeat(N // UNIQUE)
    off = torch.arange(N, dtype=torch.int64, device=dev) * stride
    ln = torch.full((N,), len(entries[0]), dtype=torch.int32, device=dev)
    return d_in, off, ln


datas = [rnd.bytes(SIZE) for _ in range(UNIQUE)]
d_out = torch.empty(N * SIZE, dtype=torch.uint8, device=dev)
out_off = torch.arange(N, dtype=torch.int64, device=dev) * SIZE
r_len, r_st = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
want = torch.from_numpy(np.frombuffer(b"".join(datas), dtype=np.uint8).copy()).to(dev)

d_in, off, ln = resident([cr.pk_encrypt(PW, d, 1, 2, header_seed=i) for i, d in enumerate(datas)])
ver = torch.full((N,), 2, dtype=torch.int32, device=dev)


def pk():
    assert L.mzhip_pkcrypt_batch(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), d_out.data_ptr(), out_off.data_ptr(), N, PW, len(PW),
                                 ver.data_ptr(), r_len.data_ptr(), r_st.data_ptr(), None) == 0


ms = timed(pk)
ok = bool((r_st == 0).all()) and bool((d_out[:UNIQUE * SIZE] == want).all()) and bool((d_out[-UNIQUE * SIZE:] == want).all())
print("ZipCrypto  k_pkcrypt_batch: %d x %d B: %.2f ms  %.1f GiB/s  ok=%s" % (N, SIZE, ms, GIB / (ms / 1e3), ok), flush=True)
del d_in

d_in, off, ln = resident([cr.wz_encrypt(PW, d, STRENGTH, salt_seed=i) for i, d in enumerate(datas)])
strength = torch.full((N,), STRENGTH, dtype=torch.uint8, device=dev)
d_out.zero_()


def aes(pw):
    assert L.mzhip_wzaes_batch(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), strength.data_ptr(), d_out.data_ptr(), out_off.data_ptr(),
                               N, pw, len(pw), r_len.data_ptr(), r_st.data_ptr(), None) == 0


ms = timed(lambda: aes(PW))
ok = bool((r_st == 0).all()) and bool((d_out[:UNIQUE * SIZE] == want).all()) and bool((d_out[-UNIQUE * SIZE:] == want).all())
print("WinZip AES-%d keys + CTR + auth: %d x %d B: %.2f ms  %.1f GiB/s  ok=%s" % (64 + 64 * STRENGTH, N, SIZE, ms, GIB / (ms / 1e3), ok),
      flush=True)
ms = timed(lambda: aes(b"test124"))
print("WinZip AES wrong password (k_wzaes_keys alone has work): %.2f ms = %.2f us per entry  all refused=%s"
      % (ms, ms * 1e3 / N, bool((r_st == cr.MZ_PASSWORD_ERROR).all())), flush=True)
