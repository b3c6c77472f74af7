"""GPU test of two parts of K1 (minizip-ng_amd/csrc): the chase of pass 2 that takes its next target in front of a trip
(inflate_walk.inc, MZ_CHASE_RETARGET) and the near batches' set-up (inflate_commit.inc, the rank searches).  The cases of
tests/chase_lean_cases.py -- small entries whose chases run through whole spans, block ends and record caps inside chases, every
short distance with every piece length at every staging phase -- repeated at other misalignments to a few thousand entries in
ONE launch of mzhip_inflate_batch, and once more through mzhip_inflate_resume_batch (k_inflate_batch<true>, another compile of
the same sources); then 256 entries of 64 KiB of the benchmark's corpus through both.  The entries are laid out byte by byte
with a red zone of pattern between them, so inputs and outputs take every misalignment 0 .. 15.  zlib is the judge of status,
out_len, in_used, bytes and CRC.

Caps of this file: four launches, 2 642 + 256 entries, 32 MiB of output slots."""
import time
import zlib

import numpy as np
import pytest

from tests import chase_lean_cases as CL

pytestmark = pytest.mark.gpu

GUARD = 64
REPEAT = 20


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


@pytest.fixture(scope="module")
def small():
    """[(name, stream, bytes, cap)]: every case REPEAT times in a seeded order (other neighbours, other misalignments), the two
    long ones once; zlib's verdict asserted of each case"""
    import random

    cases = CL.everything()
    for name, z, data, cap in cases:
        d = zlib.decompressobj(-15)
        assert d.decompress(z) == data and d.eof and d.unused_data == b"", name
    out = [c for c in cases for _ in range(REPEAT if len(c[2]) <= 40000 else 1)]
    random.Random(77).shuffle(out)
    assert 2000 <= len(out) <= 4096
    return out


@pytest.fixture(scope="module")
def corpus64():
    """256 entries of 64 KiB of the benchmark's corpus at level 6"""
    from tests import synth

    text = synth.bench_corpus()[0]
    out = []
    for i in range(256):
        o = (i * 104729) % (len(text) - 65536)
        d = bytes(text[o:o + 65536])
        out.append(("corpus64/%d" % i, synth.deflate_raw(d), d, 65536))
    return out


def _check(gpu, what, entries, batch, res):
    out_len, in_used, crc, status = res
    h_out = gpu.check_guards(batch, out_len, status)
    for i, (name, z, data, cap) in enumerate(entries):
        assert status[i] == 0, (what, name, int(status[i]))
        assert out_len[i] == len(data) and in_used[i] == len(z), (what, name, int(out_len[i]), len(data), int(in_used[i]), len(z))
        got = gpu.entry_bytes(batch, h_out, i, len(data))
        if got != data:
            bad = next(k for k in range(len(data)) if got[k] != data[k])
            raise AssertionError("%s: %s: byte %d of %d is %d, zlib says %d" % (what, name, bad, len(data), got[bad], data[bad]))
        assert int(crc[i]) == zlib.crc32(data), (what, name)


def _both_kernels(gpu, what, entries):
    from tests.test_gpu_bounds import launch_inflate

    batch = gpu.make_batch([e[1] for e in entries], [e[3] for e in entries], align=1, guard=GUARD, fill=77)
    _check(gpu, what + "/batch", entries, batch, gpu.run_inflate(batch))
    batch = gpu.make_batch([e[1] for e in entries], [e[3] for e in entries], align=1, guard=GUARD, fill=78)
    R = launch_inflate(gpu, batch, stop=True)
    n = batch["n"]
    res = (gpu.result_words(R["out_len"], n).astype(np.int64), gpu.result_words(R["in_used"], n).astype(np.int64),
           gpu.result_words(R["crc"], n), gpu.result_words(R["status"], n).view(np.int32))
    _check(gpu, what + "/resumable", entries, batch, res)
    return batch


def test_small_entries_both_kernels(gpu, small):
    t0 = time.time()
    batch = _both_kernels(gpu, "small", small)
    assert {int(o) % 16 for o in batch["h_in_off"]} == set(range(16))
    print("test_small_entries_both_kernels: 2 launches of %d entries, %.2f s" % (len(small), time.time() - t0))


def test_bench_corpus_64k_both_kernels(gpu, corpus64):
    t0 = time.time()
    _both_kernels(gpu, "corpus64", corpus64)
    print("test_bench_corpus_64k_both_kernels: 2 launches of %d entries, %.2f s" % (len(corpus64), time.time() - t0))
