"""GPU test of the refill of K1's two walks (minizip-ng_amd/csrc/inflate_walk.inc): the cases of tests/walk_refill_cases.py --
level-6 streams whose ends take every phase of a group of four dwords, every one of them cut at every byte of its last 48, and
the two wide-step programs (63-bit steps, sustained over whole spans and in runs between 1-bit literals) -- in ONE launch of
mzhip_inflate_batch of the product build.  The entries are laid out byte by byte with a red zone of pattern between them, so
that the input pointers take every misalignment 0 .. 15, and every entry has its own guarded output slot.  zlib is the judge
of status, out_len, in_used, bytes and CRC; the host emulation of the same sources must say the same.  (That no byte behind the
input's last aligned dword is read is the sanitised CPU program's to show, tests/test_walk_refill_emul.py: the device cannot
tell.)

Caps of this file: one launch, 835 entries, 7.1 MiB of output slots."""
import ctypes as C
import time
import zlib

import numpy as np
import pytest

from tests import walk_refill_cases as W

pytestmark = pytest.mark.gpu

GUARD = 64
_u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


@pytest.fixture(scope="module")
def emu():
    """the host emulation of K1 alone, the product build (tests/emul/k1_walk_main.cpp as a library)"""
    from tests.test_walk_refill_emul import _build_variant

    return _build_variant("product", [])


def test_walk_refill_batch(gpu, emu):
    t0 = time.time()
    cases = W.everything()
    assert sum(c[3] == 0 for c in cases) == 19 and sum(c[3] == -5 for c in cases) == 17 * W.CUT_BYTES
    batch = gpu.make_batch([c[1] for c in cases], [c[5] for c in cases], align=1, guard=GUARD, fill=77)
    assert batch["d_in"].data_ptr() % 16 == 0
    assert {int(o) % 16 for o in batch["h_in_off"]} == set(range(16))                       # every misalignment of the input
    assert {(int(o) % 4 + len(c[1])) % 16 for o, c in zip(batch["h_in_off"], cases)} == set(range(16))   # every phase of its end
    last = len(cases) - 1
    assert batch["h_in"].size - (int(batch["h_in_off"][last]) + len(cases[last][1])) >= 64   # pattern behind the last input
    assert (batch["h_in"][-64:] != 0).all()
    out_len, in_used, crc, status = gpu.run_inflate(batch)
    h_out = gpu.check_guards(batch, out_len, status)
    for i, (name, z, data, want, used, cap) in enumerate(cases):
        assert status[i] == want, (name, int(status[i]), want)
        # the emulation from the same bytes at the same misalignment, non-zero bytes behind them
        mis = int(batch["h_in_off"][i]) % 16
        a = np.full(mis + len(z) + 64, 0xC3, dtype=np.uint8)
        a[mis:mis + len(z)] = np.frombuffer(z, dtype=np.uint8)
        o = np.zeros(max(cap, 1), dtype=np.uint8)
        ol, iu, cr = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = emu.emul_inflate(C.cast(a.ctypes.data + mis, _u8p), len(z), C.cast(o.ctypes.data, _u8p), cap, C.byref(ol), C.byref(iu), C.byref(cr))
        assert st == status[i], (name, st, int(status[i]))
        if want != 0:
            continue
        assert out_len[i] == len(data) == ol.value and in_used[i] == used == iu.value, (name, int(out_len[i]), len(data), int(in_used[i]), used)
        got = gpu.entry_bytes(batch, h_out, i, len(data))
        if got != data:
            bad = next(k for k in range(len(data)) if got[k] != data[k])
            raise AssertionError("%s: byte %d of %d is %d, zlib says %d" % (name, bad, len(data), got[bad], data[bad]))
        assert o[:ol.value].tobytes() == data, name
        assert int(crc[i]) == zlib.crc32(data) == cr.value, name
    print("test_walk_refill_batch: one launch of %d entries, %.2f s" % (len(cases), time.time() - t0))
