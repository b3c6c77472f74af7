"""GPU probe (not a pytest): throughput of the encrypting crypt calls at 65 536 x 64 KiB, device-resident, and -- in the same run,
on the same entries -- of the read-side calls that take them back.
Usage: python tests/perf_crypt_enc.py [n_entries]         HIP-event times of the four C ABI calls
       python tests/perf_crypt_enc.py --stats kernel_stats.csv [n_entries]
                                                          GiB/s per kernel from the `rocprofv3 --kernel-trace --stats` table
                                                          of a run of the first form
Sixteen distinct plaintexts are replicated in HBM, so every entry's bytes are read from memory.  CTR does the same work in both
directions: a large gap between k_wzaes_enc_ctr and k_wzaes_ctr points at the store side (the ciphertext lies 4 s + 6 bytes
off the input's alignment)."""
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
KERNELS = ("k_pkcrypt_enc_batch", "k_wzaes_enc_keys", "k_wzaes_enc_ctr", "k_wzaes_enc_auth", "k_pkcrypt_batch", "k_wzaes_keys",
           "k_wzaes_ctr", "k_wzaes_auth")

if stats:
    with open(stats) as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        avg = float(r.get("AverageNs") or r.get("Average") or 0)
        for k in KERNELS:
            if name.split("(")[0].strip() == k and avg:
                print("%-20s %4s calls  %9.3f ms average  %8.1f GiB/s of payload" % (k, r.get("Calls", "?"), avg / 1e6, GIB / (avg / 1e9)))
    sys.exit(0)

import torch  # noqa: E402

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


def report(what, ms, ok):
    print("%-44s %d x %d B: %9.2f ms  %8.1f GiB/s  ok=%s" % (what, N, SIZE, ms, GIB / (ms / 1e3), ok), flush=True)


plain = torch.from_numpy(np.frombuffer(rnd.bytes(UNIQUE * SIZE), dtype=np.uint8).copy()).to(dev).repeat(N // UNIQUE)
p_off = torch.arange(N, dtype=torch.int64, device=dev) * SIZE
p_len = torch.full((N,), SIZE, dtype=torch.int32, device=dev)
back = torch.empty(N * SIZE, dtype=torch.uint8, device=dev)
r_len, r_st = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
noise = torch.from_numpy(np.frombuffer(rnd.bytes(16 * N), dtype=np.uint8).copy()).to(dev)

for kind in ("pk", "aes"):
    over = 12 if kind == "pk" else 4 * STRENGTH + 16
    stride = (SIZE + over + 63) // 64 * 64
    enc = torch.empty(N * stride, dtype=torch.uint8, device=dev)
    e_off = torch.arange(N, dtype=torch.int64, device=dev) * stride
    e_len = torch.zeros(N, dtype=torch.int32, device=dev)
    ver = torch.full((N,), 0x0102, dtype=torch.int32, device=dev)
    strength = torch.full((N,), STRENGTH, dtype=torch.uint8, device=dev)

    def encrypt():
        if kind == "pk":
            rc = L.mzhip_pkcrypt_encrypt_batch(plain.data_ptr(), p_off.data_ptr(), p_len.data_ptr(), enc.data_ptr(), e_off.data_ptr(), N,
                                               PW, len(PW), ver.data_ptr(), noise.data_ptr(), e_len.data_ptr(), r_st.data_ptr(), None)
        else:
            rc = L.mzhip_wzaes_encrypt_batch(plain.data_ptr(), p_off.data_ptr(), p_len.data_ptr(), strength.data_ptr(), noise.data_ptr(),
                                             enc.data_ptr(), e_off.data_ptr(), N, PW, len(PW), e_len.data_ptr(), r_st.data_ptr(), None)
        assert rc == 0

    def decrypt():
        if kind == "pk":
            rc = L.mzhip_pkcrypt_batch(enc.data_ptr(), e_off.data_ptr(), e_len.data_ptr(), back.data_ptr(), p_off.data_ptr(), N, PW,
                                       len(PW), ver.data_ptr(), r_len.data_ptr(), r_st.data_ptr(), None)
        else:
            rc = L.mzhip_wzaes_batch(enc.data_ptr(), e_off.data_ptr(), e_len.data_ptr(), strength.data_ptr(), back.data_ptr(),
                                     p_off.data_ptr(), N, PW, len(PW), r_len.data_ptr(), r_st.data_ptr(), None)
        assert rc == 0

    name = "ZipCrypto" if kind == "pk" else "WinZip AES-%d" % (64 + 64 * STRENGTH)
    ms = timed(encrypt)
    report(name + (" encrypt (k_pkcrypt_enc_batch)" if kind == "pk" else " encrypt (keys + CTR + auth)"), ms,
           bool((r_st == 0).all()) and bool((e_len == SIZE + over).all()))
    back.zero_()
    ms = timed(decrypt)
    report(name + " decrypt of the same entries", ms,
           bool((r_st == 0).all()) and bool((r_len == SIZE).all()) and bool((back == plain).all()))
    del enc
