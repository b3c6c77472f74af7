"""GPU tests of the synchronous one-entry host-buffer calls (what the drop-in shims call for an entry that is not primed):
a whole-entry decode through a host call gives what the batch launcher of the same library gives for a batch of one
(methods 8, 14, 95 and 12: status, out_len, in_used, crc and bytes, at sizes around the staging buffer's 16- and 64-byte
paddings and the 64 KiB block; trailing bytes, a cut stream, out_cap exact and one short, a guard behind out_cap, null
result pointers, a null output); the whole-entry LZMA encoder against liblzma, zlib.crc32 and its OUT_FULL rule; and the two
.xz writers -- a whole stream in one call, a block and the index / footer call -- byte for byte.
Streams come from CPython's zlib, lzma and bz2; signatures from include/mzhip.h (minizip-ng_amd.lib())."""
import bz2
import ctypes as C
import lzma
import zlib

import numpy as np
import pytest

from tests import gpu_util, synth
from tests.test_oracle import _zip_lzma

pytestmark = pytest.mark.gpu
mz = gpu_util.mz

SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 65535, 65536, 65537]
GUARD = 8
OUT_FULL = -200  # MZHIP_STATUS_OUT_FULL


@pytest.fixture(scope="module")
def gpu():
    import torch

    mz.require_gpu()
    torch.cuda.set_device(0)
    return gpu_util


def text(n):
    return synth.corpus()[1000:1000 + n]


def pattern(n, seed=7):
    return gpu_util.guard_pattern(n, seed).tobytes()


# method -> (stream maker, batch launcher, takes max_out)
CODECS = {
    8: (synth.deflate_raw, "mzhip_inflate_batch", False),
    14: (_zip_lzma, "mzhip_lzma_batch", True),
    95: (lambda d: lzma.compress(d, format=lzma.FORMAT_XZ), "mzhip_xz_batch", True),
    12: (bz2.compress, "mzhip_bzip2_batch", False),
}


def batch_of_one(method, z, cap):
    """-> (status, out_len, in_used, crc, bytes) of the batch launcher, n = 1; result words start as zero, as a host call's do"""
    import torch

    _, name, family = CODECS[method]
    b = gpu_util.make_batch([z], [cap])
    res = [torch.zeros(1, dtype=torch.int32, device=b["d_in"].device) for _ in range(4)]
    mo = torch.tensor([-1], dtype=torch.int64, device=b["d_in"].device)
    args = [b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), b["d_out"].data_ptr(), b["out_off"].data_ptr(),
            b["out_cap"].data_ptr()] + ([mo.data_ptr()] if family else []) + [1] + [t.data_ptr() for t in res] + [None]
    rc = getattr(mz.lib(), name)(*args)
    assert rc == 0, (name, rc, mz.lib().mzhip_last_error())
    torch.cuda.synchronize()
    out_len, in_used, crc, status = (int(mz.u32(t)[0]) for t in res)
    status = int(res[3].cpu().numpy()[0])
    return status, out_len, in_used, crc, gpu_util.entry_bytes(b, b["d_out"].cpu().numpy(), 0, min(out_len, cap))


def host_call(method, z, cap, results=True, adler=False, out=True):
    """-> (status, out_len, in_used, crc, bytes[, adler]) of the host call; the 8 bytes behind out_cap must come back untouched"""
    L = mz.lib()
    fill = pattern(cap + GUARD)
    buf = C.create_string_buffer(fill, cap + GUARD) if out else None
    ol, iu, crc, ad = (C.c_uint32(0) for _ in range(4))
    p = [C.addressof(v) if results else None for v in (ol, iu, crc)]
    if method == 8:
        src = C.create_string_buffer(z, max(len(z), 1))
        a = mz.InflateHostArgs(size=C.sizeof(mz.InflateHostArgs), in_len=len(z), buf_cap=cap, in_=C.addressof(src),
                               buf=C.addressof(buf) if out else None, out_len=p[0], in_used=p[1], crc=p[2],
                               adler=C.addressof(ad) if adler else None)
        st = L.mzhip_inflate_host_a(C.byref(a))
    elif method == 12:
        st = L.mzhip_bzip2_host(z, len(z), buf, cap, *p)
    else:
        st = (L.mzhip_lzma_host if method == 14 else L.mzhip_xz_host)(z, len(z), buf, cap, -1, *p)
    if out:
        assert buf.raw[cap:] == fill[cap:], "bytes behind out_cap were written"
    r = (int(st), ol.value, iu.value, crc.value, buf.raw[:min(ol.value, cap)] if out else b"")
    return r + (ad.value,) if adler else r


@pytest.fixture(scope="module")
def streams():
    return {(m, n): CODECS[m][0](text(n)) for m in CODECS for n in SIZES}


@pytest.mark.parametrize("method", sorted(CODECS))
def test_host_call_equals_batch_of_one(gpu, streams, method):
    for n in SIZES:
        d, z = text(n), streams[method, n]
        variants = [("plain", z, n + 8), ("trailing", z + b"\x00tail", n + 8), ("cut", z[:len(z) // 2], n + 8), ("exact", z, n)]
        if n:
            variants.append(("short", z, n - 1))
        for name, zz, cap in variants:
            h, b = host_call(method, zz, cap), batch_of_one(method, zz, cap)
            assert h[:4] == b[:4], (method, n, name, h[:4], b[:4])
            assert h[4] == b[4], (method, n, name)
            if h[0] == 0:
                assert h[4] == d and h[3] == zlib.crc32(d), (method, n, name)
            if name == "plain" and (n or method == 8):  # (an empty method-12, -14 or -95 payload is what the batch makes of it)
                assert h[0] == 0 and h[2] == len(zz), (method, n, h[:4])
            if name == "trailing" and h[0] == 0:
                assert h[2] <= len(z) < len(zz), (method, n, h[2])
            if name == "short":
                assert h[0] != 0, (method, n)


def test_inflate_adler_is_zlibs(gpu, streams):
    for n in SIZES:
        st, ol, iu, crc, out, ad = host_call(8, streams[8, n], n + 8, adler=True)
        d = text(n)
        assert (st, ol, iu, crc, out) == (0, n, len(streams[8, n]), zlib.crc32(d), d) and ad == zlib.adler32(d), n


@pytest.mark.parametrize("method", sorted(CODECS))
def test_null_result_pointers_and_null_output(gpu, streams, method):
    for n in (0, 17, 65537):
        z = streams[method, n]
        for cap in (n + 8, n - 1) if n else (8,):
            assert host_call(method, z, cap, results=False)[0] == host_call(method, z, cap)[0], (method, n, cap)
    # out == NULL with out_cap == 0 on the stream of no bytes
    assert host_call(method, streams[method, 0], 0, out=False)[:4] == batch_of_one(method, streams[method, 0], 0)[:4]
    assert host_call(method, streams[method, 0], 0, out=False, results=False)[0] == batch_of_one(method, streams[method, 0], 0)[0]


def _alone(z):
    return z[4:9] + b"\xff" * 8 + z[9:]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 65536, 65537])
def test_whole_entry_lzma_encode(gpu, n):
    L = mz.lib()
    d = text(n)
    cap = n + n // 8 + 2048
    out = C.create_string_buffer(cap)
    ol, crc = C.c_uint32(0), C.c_uint32(0)
    assert L.mzhip_lzma_encode_host_preset(d, n, 6, out, cap, C.byref(ol), C.byref(crc)) == 0
    z = out.raw[:ol.value]
    assert lzma.decompress(_alone(z), format=lzma.FORMAT_ALONE) == d and crc.value == zlib.crc32(d)
    # one byte short: OUT_FULL, the length that is needed, and nothing copied
    fill = pattern(len(z) - 1 + GUARD)
    small = C.create_string_buffer(fill, len(fill))
    ol2 = C.c_uint32(0)
    assert L.mzhip_lzma_encode_host_preset(d, n, 6, small, len(z) - 1, C.byref(ol2), None) == OUT_FULL
    assert ol2.value == len(z) and small.raw == fill


@pytest.mark.parametrize("preset", [1, 6])
def test_xz_writers_agree(gpu, preset):
    L = mz.lib()
    for n in (1, 65536, 65537, 200000):
        d = text(n)
        cap = n + n // 8 + 4096
        a, b = C.create_string_buffer(cap), C.create_string_buffer(cap)
        la, ca, lb, cb, lt = (C.c_uint32(0) for _ in range(5))
        assert L.mzhip_xz_encode_host_preset(d, n, preset, a, cap, C.byref(la), C.byref(ca)) == 0
        unpadded, size = C.c_uint64(0), C.c_uint64(n)
        assert L.mzhip_xz_encode_block_host(d, n, preset, 1, b, cap, C.byref(lb), C.byref(cb), C.byref(unpadded)) == 0
        tail = C.create_string_buffer(64)
        assert L.mzhip_xz_encode_finish_host(C.byref(unpadded), C.byref(size), 1, tail, 64, C.byref(lt)) == 0
        A, B = a.raw[:la.value], b.raw[:lb.value] + tail.raw[:lt.value]
        assert A == B, (n, preset, len(A), len(B))
        assert ca.value == cb.value == zlib.crc32(d)
        assert lzma.decompress(A, format=lzma.FORMAT_XZ) == d
        assert L.mzhip_xz_encode_finish_host(C.byref(unpadded), C.byref(size), 1, tail, lt.value - 1, None) == OUT_FULL
