"""GPU tests of what the LZMA encoder (K6) promises about the STRUCTURE of its output, read packet by packet with
tests/lzma_tokens.py -- a decoder that gets the input back cannot see any of it:
  - reach (include/mzhip.h, mzhip_lzma_encode_history_bytes): matches reach back history_bytes() - 1 bytes and no further,
    32 KiB in a stream of one block; the echo the reach just allows is USED -- the chain pass (lzma_enc_core.h mz_lz_chain)
    rests on device-scope atomics and L2-coherent loads that the host emulation does not have, and a stale table read costs
    only matches, never validity;
  - seams: no packet covers bytes on both sides of a multiple of 64 KiB (the .xz writer makes one LZMA2 chunk of each);
  - framing: the nine header bytes and their dictionary, the one end marker, a coder that ends on its last byte, the LZMA2
    control bytes, chunk sizes and stored chunks, the block header's dictionary byte;
  - determinism: the device's bytes are the host emulation's for the same parse class and chain depth, byte for byte.
The same asserts run on the 64-lane emulation in tests/test_lzma_tokens.py; here the wave-level code is the real thing."""
import ctypes as C
import lzma
import zlib

import numpy as np
import pytest

from tests import lzma_packets, lzma_tokens as T, synth
from tests.test_lzma_tokens import depth_for_preset, emul_encode, is_far_sized

pytestmark = pytest.mark.gpu
PRESETS = (1, 6, 9)
NEAR_COVER = ("near/32767", "near/32768")
_u32p = C.POINTER(C.c_uint32)


class EncState(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("flags", "low_lo", "low_hi", "range", "cache", "cache_size", "state", "rep0", "rep1", "rep2", "rep3")] + [("pad", C.c_uint32 * 5)]


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    L = gpu_util.mz.lib()
    L.mzhip_lzma_encode_batch_preset.restype = C.c_int32
    L.mzhip_lzma_encode_batch_preset.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_int32] + [C.c_void_p] * 4
    for f in (L.mzhip_lzma_encode_host_preset, L.mzhip_xz_encode_host_preset):
        f.restype = C.c_int32
        f.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint32, _u32p, _u32p]
    L.mzhip_lzma_encode_history_bytes.restype = C.c_uint32
    L.mzhip_lzma_encode_history_bytes.argtypes = []
    L.mzhip_lzma_model_bytes.restype = C.c_uint32
    L.mzhip_lzma_model_bytes.argtypes = []
    L.mzhip_xz_encode_block_host.restype = C.c_int32
    L.mzhip_xz_encode_block_host.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, _u32p, _u32p, C.POINTER(C.c_uint64)]
    L.mzhip_xz_encode_finish_host.restype = C.c_int32
    L.mzhip_xz_encode_finish_host.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p, C.c_uint32, _u32p]
    L.mzhip_lzma_encode_resume_host.restype = C.c_int32
    L.mzhip_lzma_encode_resume_host.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(EncState), C.POINTER(EncState), C.c_void_p,
                                                C.c_void_p, C.c_uint32, _u32p]
    return gpu_util


def _far(gpu):
    return int(gpu.mz.lib().mzhip_lzma_encode_history_bytes())


def _cases(gpu):
    return synth.lzma_echo_cases(_far(gpu))


_BATCH = {}


def _batch(gpu, preset):
    """ONE mzhip_lzma_encode_batch_preset launch with every case as an entry -> {name: bytes}; status 0 and the CRC of the
    input asserted per entry.  max_in_len exceeds one block while some entries are one block: that mix is itself a case."""
    if preset in _BATCH:
        return _BATCH[preset]
    import torch

    cases = _cases(gpu)
    datas = [c[1] for c in cases]
    caps = [len(d) + len(d) // 8 + 1024 for d in datas]
    b = gpu.make_batch(datas, caps)
    n = len(datas)
    dev = b["d_in"].device
    out_len, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    rc = gpu.mz.lib().mzhip_lzma_encode_batch_preset(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), max(len(d) for d in datas),
                                                     b["d_out"].data_ptr(), b["out_off"].data_ptr(), b["out_cap"].data_ptr(), None, n, preset,
                                                     out_len.data_ptr(), crc.data_ptr(), status.data_ptr(), None)
    assert rc == 0, (preset, rc)
    torch.cuda.synchronize()
    h = b["d_out"].cpu().numpy()
    ol, st, k = out_len.cpu().numpy(), status.cpu().numpy(), gpu.mz.u32(crc)
    res = {}
    for i, (name, d, _) in enumerate(cases):
        assert st[i] == 0 and k[i] == zlib.crc32(d), (preset, name, int(st[i]))
        res[name] = gpu.entry_bytes(b, h, i, int(ol[i]))
    _BATCH[preset] = res
    return res


def _host(fn, d, preset):
    cap = len(d) + len(d) // 8 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    ol, crc = C.c_uint32(), C.c_uint32()
    assert fn(d, len(d), preset, out.ctypes.data, cap, C.byref(ol), C.byref(crc)) == 0, (len(d), preset)
    assert crc.value == zlib.crc32(d), (len(d), preset)
    return out[:ol.value].tobytes()


@pytest.mark.parametrize("preset", PRESETS)
def test_batch_packets(gpu, preset):
    """every entry of the launch: lzma_tokens.check_encoded -- header and dictionary, the bytes, the one end marker, code 0 on
    the last byte, lengths, no short rep, no match at a rep distance, no short copy from beyond 32 KiB, every distance within
    the reach, the echo at the reach taken and the one beyond it not, no packet across a seam; liblzma reads every entry."""
    far = _far(gpu)
    zs = _batch(gpu, preset)
    for name, d, period in _cases(gpu):
        where = ("preset %d" % preset, name)
        T.check_encoded(zs[name], d, preset <= 3, far, where=where, period=period, near_cover=name in NEAR_COVER)
        assert lzma.decompress(zs[name][4:9] + b"\xff" * 8 + zs[name][9:], format=lzma.FORMAT_ALONE) == d, where


def _same_as_emulation(z, d, preset, where):
    """the device's stream is the emulation's for the preset's class; where the device does not grant the tokenizer its
    128 KiB of LDS the launcher falls back to the one-way class at the preset's chain depth -- said, not silently taken"""
    ways = 1 if preset <= 3 else 4
    depth = depth_for_preset(preset)
    if emul_encode(d, ways, depth) == z:
        return
    if ways > 1 and emul_encode(d, 1, depth) == z:
        print("%s: the device fell back to the ONE-WAY class (no 128 KiB of LDS for the tokenizer); its stream is the emulation's for that class" % (where,))
        return
    want = emul_encode(d, ways, depth)
    first = next((i for i in range(min(len(z), len(want))) if z[i] != want[i]), min(len(z), len(want)))
    raise AssertionError((where, "the device's stream is not the emulation's: %d and %d bytes, the first difference at byte %d" % (len(z), len(want), first)))


@pytest.mark.parametrize("preset", PRESETS)
def test_batch_equals_emulation(gpu, preset):
    """lzma_enc_core.h calls the chain pass deterministic (the table takes positions by atomic maximum and is read where the
    atomics land): the device's bytes are the emulation's, for every case but the three far-sized ones (below)"""
    far = _far(gpu)
    zs = _batch(gpu, preset)
    for name, d, _ in _cases(gpu):
        if not is_far_sized(name, far):
            _same_as_emulation(zs[name], d, preset, ("preset %d" % preset, name))


@pytest.mark.parametrize("which", (-1, 0, 1), ids=("far-1", "far", "far+1"))
@pytest.mark.parametrize("preset", (1, 6))
def test_batch_equals_emulation_far_sized(gpu, preset, which):
    """the same for the far-sized cases (8.4 MB each, seconds in emulation): a test of its own each, one preset per class"""
    far = _far(gpu)
    name = "far/%d" % (far + which)
    d = next(c[1] for c in _cases(gpu) if c[0] == name)
    _same_as_emulation(_batch(gpu, preset)[name], d, preset, ("preset %d" % preset, name))


def test_host_entry_point_makes_the_batch_bytes(gpu):
    """mzhip_lzma_encode_host_preset on the far and seam cases: the bytes of the batch launch"""
    L = gpu.mz.lib()
    far = _far(gpu)
    for preset in PRESETS:
        zs = _batch(gpu, preset)
        for name, d, _ in _cases(gpu):
            if name.startswith("far/") and (preset == 6 or not is_far_sized(name, far)):
                assert _host(L.mzhip_lzma_encode_host_preset, d, preset) == zs[name], (preset, name)


@pytest.mark.parametrize("preset", (1, 6))
def test_xz_host_chunks(gpu, preset):
    """mzhip_xz_encode_host_preset over the same cases: lzma_tokens.check_xz -- block header and dictionary byte, chunk
    layout, control bytes, sizes, a coder per chunk that ends on code 0 with its last byte, the packet rules over the block
    (a far echo across chunks is used), the container as liblzma accepts it; the block of noise is stored, the text behind
    it coded."""
    L = gpu.mz.lib()
    far = _far(gpu)
    for name, d, period in _cases(gpu):
        where = ("xz preset %d" % preset, name)
        x = _host(L.mzhip_xz_encode_host_preset, d, preset)
        xw = T.check_xz(x, d, far, where=where, period=period, near_cover=name in NEAR_COVER)
        if name == "noise+text":
            assert [c.control for c in xw.blocks[0].walk.chunks] == [0x01, 0xC0], where


def test_xz_block_then_finish(gpu):
    """mzhip_xz_encode_block_host with first = 1, then mzhip_xz_encode_finish_host, on the echo across sixteen blocks: the same
    chunk rules, and liblzma reads the stream"""
    L = gpu.mz.lib()
    far = _far(gpu)
    name, d, period = next(c for c in _cases(gpu) if c[0] == "far/%d" % (16 * 65536 - 2000))
    for preset in (1, 6):
        cap = len(d) + len(d) // 8 + 4096
        out = np.zeros(cap, dtype=np.uint8)
        ol, crc, unp = C.c_uint32(), C.c_uint32(), C.c_uint64()
        assert L.mzhip_xz_encode_block_host(d, len(d), preset, 1, out.ctypes.data, cap, C.byref(ol), C.byref(crc), C.byref(unp)) == 0
        assert crc.value == zlib.crc32(d)
        tail = np.zeros(256, dtype=np.uint8)
        tl, unc = C.c_uint32(), C.c_uint64(len(d))
        assert L.mzhip_xz_encode_finish_host(C.byref(unp), C.byref(unc), 1, tail.ctypes.data, 256, C.byref(tl)) == 0
        x = out[:ol.value].tobytes() + tail[:tl.value].tobytes()
        where = ("xz block + finish, preset %d" % preset, name)
        xw = T.walk_xz(x)
        assert len(xw.blocks) == 1 and xw.blocks[0].unpadded_size == unp.value and xw.data == d, where
        T.check_block(xw.blocks[0], d, far, where, period, False, lzma_packets.lzma2_dict_byte(far))
        assert lzma.decompress(x, format=lzma.FORMAT_XZ) == d, where


def test_resume_segments_make_the_one_shot_bytes(gpu):
    """mzhip_lzma_encode_resume_host called directly (otherwise reached through the drop-in library alone): a stream written
    in segments of two blocks, the caller keeping min(coded so far, history_bytes()) in front of each as include/mzhip.h
    describes -- the concatenated segments are mzhip_lzma_encode_host_preset's bytes and pass check_encoded"""
    L = gpu.mz.lib()
    far = _far(gpu)
    seg = 2 * 65536
    echo = next(c for c in _cases(gpu) if c[0] == "far/%d" % (16 * 65536 - 2000))
    for name, d, period in (echo, ("text/%d" % (5 * 65536 + 777), synth.corpus()[:5 * 65536 + 777], None)):
        for preset in (1, 6):
            model = np.zeros(L.mzhip_lzma_model_bytes(), dtype=np.uint8)
            st_in, st_out = EncState(), EncState()
            z = b""
            for lo in range(0, len(d), seg):
                hi = min(lo + seg, len(d))
                hist = min(lo, far) // 65536 * 65536
                buf = d[lo - hist:hi]
                cap = (hi - lo) + (hi - lo) // 8 + 4096
                out = np.zeros(cap, dtype=np.uint8)
                ol = C.c_uint32()
                last = 1 if hi == len(d) else 0
                st_in.flags = 1 if lo else 0
                rc = L.mzhip_lzma_encode_resume_host(buf, len(buf), hist // 65536, last, preset, C.byref(st_in), C.byref(st_out), model.ctypes.data,
                                                     out.ctypes.data, cap, C.byref(ol))
                assert rc == 0, (name, preset, lo, rc)
                z += out[:ol.value].tobytes()
                st_in = st_out
                st_out = EncState()
            where = ("resume, preset %d" % preset, name)
            assert z == _host(L.mzhip_lzma_encode_host_preset, d, preset), where
            T.check_encoded(z, d, preset <= 3, far, where=where, period=period)
