"""GPU tests of K1's commit stage on the entries of tests/commit_chain_cases.py (the CPU twin on the host emulation, for
every number of CRC chains, is tests/test_commit_chains_emul.py): output sizes on, before and behind every group
boundary of the CRC fold, and near-copy tails of every length at the distances next to 1 .. 8, 16 and 32 -- through
mzhip_inflate_batch in one launch (byte by byte, and packed with every 16-byte misalignment of the output), and the sizes
once more through the resumable path in two calls, so that the CRC of the second call starts behind history
(crc_base != 0).  zlib judges the bytes, zlib.crc32 the CRC.

Caps of this file: at most 4096 entries and 32 MiB of expected output per launch."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import commit_chain_cases as cases

pytestmark = pytest.mark.gpu

MAX_ENTRIES, MAX_LAUNCH_BYTES = 4096, 32 << 20


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


def _launch_and_check(gpu, what, entries, caps, **layout):
    assert len(entries) <= MAX_ENTRIES and sum(len(e[2]) for e in entries) <= MAX_LAUNCH_BYTES
    batch = gpu.make_batch([e[1] for e in entries], caps, **layout)
    out_len, in_used, crc, status = gpu.run_inflate(batch)
    h_out = batch["d_out"].cpu().numpy()
    for i, (name, z, data) in enumerate(entries):
        assert status[i] == 0, (what, name, int(status[i]))
        assert out_len[i] == len(data) and in_used[i] == len(z), (what, name, int(out_len[i]), len(data), int(in_used[i]), len(z))
        got = gpu.entry_bytes(batch, h_out, i, len(data))
        if got != data:
            bad = next(k for k in range(len(data)) if got[k] != data[k])
            raise AssertionError("%s: %s: byte %d of %d is %d, zlib says %d" % (what, name, bad, len(data), got[bad], data[bad]))
        assert int(crc[i]) == zlib.crc32(data), (what, name)
    return batch


def test_batch_commit_chain_entries(gpu):
    """Every entry in ONE launch laid out byte by byte (align=1), and once more packed, four copies of every entry, with
    out_cap padded so that copy j lands 5 j bytes (mod 16) off a 16-byte boundary: the launch takes all 16 misalignments
    and every entry four of them."""
    entries = cases.all_entries()
    for name, z, data in entries:                       # (the judge, of the cases themselves)
        d = zlib.decompressobj(-15)
        assert d.decompress(z) == data and d.eof and not d.unused_data, name
    _launch_and_check(gpu, "align=1", entries, [len(d) for _, _, d in entries], align=1)
    packed, caps, off = [], [], 0
    for j, e in enumerate(entries * 4):
        assert off % 16 == (5 * j) % 16
        pad = (5 * (j + 1) - (off + len(e[2]))) % 16    # the next copy starts at 5 (j + 1) mod 16
        packed.append(e)
        caps.append(len(e[2]) + pad)
        off += len(e[2]) + pad
    batch = _launch_and_check(gpu, "packed", packed, caps, packed=True)
    assert len({int(o) & 15 for o in batch["h_out_off"]}) == 16


def test_resumable_two_calls_crc_behind_history(gpu):
    """The size list through mzhip_inflate_host_a window by window: a first call with room for half of the output, a second
    one behind the history it left (at most 32 KiB): the CRC-32 of each call is that of its new bytes alone."""
    mz = gpu.mz
    L = mz.lib()
    L.mzhip_inflate_host_a.restype = C.c_int32
    L.mzhip_inflate_host_a.argtypes = [C.c_void_p]

    def call(z, buf, cap, st_in):
        st_out = (C.c_uint32 * 4)()
        ol, iu, crc = C.c_uint32(), C.c_uint32(), C.c_uint32()
        zin = np.frombuffer(z + bytes(8), dtype=np.uint8).copy()
        a = mz.InflateHostArgs(size=C.sizeof(mz.InflateHostArgs), in_len=len(z), buf_cap=cap, in_=zin.ctypes.data, buf=buf.ctypes.data,
                               state_in=C.addressof(st_in) if st_in is not None else None, state_out=C.addressof(st_out),
                               out_len=C.addressof(ol), in_used=C.addressof(iu), crc=C.addressof(crc))
        rc = L.mzhip_inflate_host_a(C.byref(a))
        return rc, ol.value, iu.value, crc.value, st_out

    behind_history = 0
    for name, z, data in cases.sizes():
        n = len(data)
        cap1 = n // 2
        buf = np.full(cap1 + 64, 0xA5, dtype=np.uint8)
        rc, n1, _, crc1, st = call(z, buf, cap1, None)
        assert (buf[cap1:] == 0xA5).all(), name
        if n == 0:
            assert (rc, n1, crc1) == (0, 0, 0), (name, rc, n1)
            continue
        assert rc == -200 and n1 <= cap1 and st[3] & 1, (name, rc, n1, cap1, list(st))
        assert buf[:n1].tobytes() == data[:n1] and crc1 == zlib.crc32(data[:n1]), name
        h = min(n1, 32768)
        cap2 = h + n - n1
        buf2 = np.full(cap2 + 64, 0xA5, dtype=np.uint8)
        buf2[:h] = np.frombuffer(data[n1 - h:n1], dtype=np.uint8)
        st_in = (C.c_uint32 * 4)(st[0], st[1], h, st[3])
        rc, n2, used, crc2, _ = call(z, buf2, cap2, st_in)
        assert (rc, n2, used) == (0, cap2, len(z)), (name, rc, n2, cap2, used, len(z))
        assert buf2[:cap2].tobytes() == data[n1 - h:] and (buf2[cap2:] == 0xA5).all(), name
        assert crc2 == zlib.crc32(data[n1:]), name
        behind_history += h != 0
    assert behind_history >= 2 * (len(cases.SIZES) - 2)   # (one stored block of the whole entry does not fit half the room: no history)
