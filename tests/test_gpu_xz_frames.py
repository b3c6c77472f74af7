"""GPU tests of the .xz container walk (xz_core.h mz_xz_entry, ZIP method 95) with the frame programs of tests/xz_frames.py:
every named program and 2000 re-sealed mutations in ONE mzhip_xz_batch launch, judged by liblzma (Python's lzma) -- status
exact; bytes, out_len, in_used and CRC-32 exact for accepted streams; in_used == in_len where liblzma wants more input;
the input unchanged, nothing outside an entry's region written, result elements behind n untouched (tests/gpu_util.py).
Then the named programs through mzhip_xz_host, out_cap one short of every accepted program, and the read() sequences of
the drop-in's mz_stream_lzma against the compiled reference.  Nothing here reads the reference's sources."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import oracle
from tests import gpu_util
from tests import xz_frames as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "integration", "_build", "libmzhipdrop.so")
GUARD = 64
SEED, N_BATCH, N_STREAMED = 1, 2000, 300
CAP_REFUSED = 4096


@pytest.fixture(scope="module")
def gpu():
    import torch

    gpu_util.mz.require_gpu()
    torch.cuda.set_device(0)
    L = gpu_util.mz.lib()
    L.mzhip_xz_batch.restype = C.c_int32
    L.mzhip_xz_batch.argtypes = [C.c_void_p] * 7 + [C.c_uint32] + [C.c_void_p] * 5
    L.mzhip_xz_host.restype = C.c_int32
    L.mzhip_xz_host.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64] + [C.POINTER(C.c_uint32)] * 3
    return gpu_util


def cases():
    """(name, stream, status, data, in_used) as liblzma judged them; the re-sealed ones are the first N_BATCH of the CPU set"""
    return F.verdicts() + [r[:5] for r in F.resealed_verdicts(SEED, 6000)[:N_BATCH]]


def launch(entries, caps, packed=False, odd=False, seed=5):
    """entries through ONE mzhip_xz_batch call, handed over in a shuffled order, inside a seeded pattern with red zones
    (packed: back to back, so every input and output alignment occurs).  check_guards holds the memory contract.
    -> (status, out_len, in_used, crc, list of output bytes), in the order of `entries`"""
    import torch

    L = gpu_util.mz.lib()
    n = len(entries)
    b = gpu_util.make_batch(entries, caps, guard=GUARD, fill=seed, packed=packed, odd=odd)
    idx = np.random.RandomState(seed).permutation(n)
    t_idx = torch.from_numpy(idx).cuda()
    d_in_off, d_in_len = b["in_off"][t_idx].contiguous(), b["in_len"][t_idx].contiguous()
    d_out_off, d_cap = b["out_off"][t_idx].contiguous(), b["out_cap"][t_idx].contiguous()
    mo = torch.full((n,), -1, dtype=torch.int64, device=b["d_in"].device)
    res = gpu_util.guarded_results(n, ["out_len", "in_used", "crc", "status"])
    rc = L.mzhip_xz_batch(b["d_in"].data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), b["d_out"].data_ptr(), d_out_off.data_ptr(),
                          d_cap.data_ptr(), mo.data_ptr(), n, res["out_len"].data_ptr(), res["in_used"].data_ptr(),
                          res["crc"].data_ptr(), res["status"].data_ptr(), None)
    assert rc == 0, (rc, L.mzhip_last_error())
    torch.cuda.synchronize()
    status, out_len, in_used, crc = (np.zeros(n, dtype=np.int64) for _ in range(4))
    status[idx] = res["status"].cpu().numpy()[:n]
    out_len[idx] = gpu_util.result_words(res["out_len"], n)
    in_used[idx] = gpu_util.result_words(res["in_used"], n)
    crc[idx] = gpu_util.result_words(res["crc"], n)
    assert (out_len <= np.asarray(caps)).all() and (in_used <= b["h_in_len"]).all()
    h_out = gpu_util.check_guards(b, out_len, status, res)
    outs = [gpu_util.entry_bytes(b, h_out, i, int(out_len[i])) for i in range(n)]
    for i in range(n):
        assert crc[i] == zlib.crc32(outs[i]), i
    return status, out_len, in_used, crc, outs


@pytest.mark.parametrize("layout", ["red_zones_odd", "packed"])
def test_programs_and_resealed_in_one_launch(gpu, layout):
    V = cases()
    caps = [len(c[3]) if c[2] == 0 else CAP_REFUSED for c in V]
    status, out_len, in_used, crc, outs = launch([c[1] for c in V], caps, packed=layout == "packed", odd=layout != "packed")
    n = {0: 0, F.DATA_ERROR: 0, F.BUF_ERROR: 0}
    part = F.partials()
    for i, (name, x, st, data, used) in enumerate(V):
        assert status[i] == st, (name, status[i], st)
        if st == 0:
            assert (out_len[i], in_used[i], crc[i]) == (len(data), used, zlib.crc32(data)) and outs[i] == data, name
        elif st == F.BUF_ERROR:
            assert in_used[i] == len(x), (name, in_used[i], len(x))
            assert name not in part or outs[i] == part[name], (name, out_len[i], len(part[name]))  # (a cut filtered block: what liblzma's chain released)
        n[st] += 1
    assert n[0] >= 150 and n[F.DATA_ERROR] >= 1500 and n[F.BUF_ERROR] >= 800, n


def test_out_cap_one_less_is_out_full(gpu):
    V = [c for c in cases() if c[2] == 0 and len(c[3]) > 0]
    status, out_len, _, _, outs = launch([c[1] for c in V], [len(c[3]) - 1 for c in V], odd=True, seed=6)
    assert len(V) >= 150 and (status == F.OUT_FULL).all(), [c[0] for c, s in zip(V, status) if s != F.OUT_FULL][:5]
    for c, o in zip(V, outs):
        assert c[3].startswith(o), c[0]


def test_host_entry_point(gpu):
    L = gpu.mz.lib()
    part = F.partials()
    for name, x, st, data, used in F.verdicts():
        cap = len(data) if st == 0 else CAP_REFUSED
        out = C.create_string_buffer(max(cap, 1) + 8)
        ol, iu, crc = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        got = L.mzhip_xz_host(x, len(x), out, cap, -1, C.byref(ol), C.byref(iu), C.byref(crc))
        assert got == st, (name, got, st)
        assert out.raw[cap:] == b"\0" * (len(out.raw) - cap), name
        if st == 0:
            assert (ol.value, iu.value, crc.value) == (len(data), used, zlib.crc32(data)) and out.raw[:ol.value] == data, name
        elif st == F.BUF_ERROR:
            assert iu.value == len(x), name
            assert out.raw[:ol.value] == part[name], (name, ol.value, len(part[name]))


@pytest.fixture(scope="module")
def libs(gpu):
    if not os.path.exists(DROP) or not oracle.have_ref():
        pytest.skip("drop-in / reference builds missing (built where /root/reference exists)")
    return oracle.MzDriver(DROP), oracle.ref()


def test_stream_reads_match_the_reference(libs):
    """the read() sequences of tests/test_xz_frames.py on the real drop-in: the named programs and 300 re-sealed mutations"""
    from tests.test_xz_frames import compare_streams, stream_cases, window_cases, window_modes

    hip, ref = libs
    diffs, first = compare_streams(hip, ref, stream_cases(N_STREAMED))
    for k in sorted(diffs):
        print(k, diffs[k], first[k])
    assert not diffs, (sum(diffs.values()), sorted(first.items())[:6])
    diffs, first = compare_streams(hip, ref, window_cases(), windows=(128 << 10,), modes=window_modes)
    assert not diffs, (sum(diffs.values()), sorted(first.items())[:6])

