"""GPU tests of what the raw-DEFLATE encoder (K4) promises about the STRUCTURE of its output, read token by token with
tests/deflate_tokens.py -- an inflater that gets the input back cannot see any of it:
  - the window (include/mzhip.h, mzhip_deflate_batch_level): no match reaches further back than 2^window_log2 - 262, at every
    level, for every window 9..15, inside one piece, into the history of a piece and through the stream shim; and the
    distance the window just allows is used;
  - the block choice (deflate_core.h: the cheapest of dynamic / fixed / stored per 64 KiB): no block larger than its bytes
    stored, random bytes stored 65535 to a block;
  - piece framing: BFINAL on the last block of a final piece only; any other piece ends on a byte boundary in 00 00 FF FF.
The same asserts run on the 64-lane emulation in tests/test_kernel_emul.py; here the wave-level code is the real thing."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import oracle
from tests import deflate_tokens, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "integration", "_build", "libmzhipdrop.so")

ALL_WINDOWS = tuple(range(9, 16))
# one level per class at every window; the other levels (their class is the same code) at the smallest and the largest
LEVEL_WINDOWS = [(1, ALL_WINDOWS), (6, ALL_WINDOWS), (9, ALL_WINDOWS)] + [(lv, (9, 15)) for lv in (0, 2, 3, 4, 5, 7, 8, -1)]


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    gpu_util.mz.lib()
    return gpu_util


def _deflate_level(gpu, datas, final, level, window_log2):
    import torch

    caps = [len(d) + len(d) // 8 + 64 for d in datas]           # exactly what include/mzhip.h says always suffices
    b = gpu.make_batch(datas, caps)
    n = len(datas)
    dev = b["d_in"].device
    out_len, crc, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    fin = torch.tensor(final, dtype=torch.uint8, device=dev)
    rc = gpu.mz.lib().mzhip_deflate_batch_level(b["d_in"].data_ptr(), b["in_off"].data_ptr(), b["in_len"].data_ptr(), b["d_out"].data_ptr(),
                                                b["out_off"].data_ptr(), b["out_cap"].data_ptr(), fin.data_ptr(), n, level, window_log2,
                                                out_len.data_ptr(), crc.data_ptr(), status.data_ptr(), None)
    assert rc == 0, (level, window_log2, rc)
    torch.cuda.synchronize()
    h = b["d_out"].cpu().numpy()
    ol = out_len.cpu().numpy()
    return [gpu.entry_bytes(b, h, i, int(ol[i])) for i in range(n)], gpu.mz.u32(crc), status.cpu().numpy()


@pytest.mark.parametrize("level,windows", LEVEL_WINDOWS, ids=["level%d" % lv for lv, _ in LEVEL_WINDOWS])
def test_batch_level_window_bound(gpu, level, windows):
    """One mzhip_deflate_batch_level launch per (level, window): synth.echo_cases(w) and synth.incompressible_cases(), final and
    non-final entries alternating (the other way round at the next window).  Per entry: status 0, the CRC of the input, and
    deflate_tokens.check_encoded -- the bytes, every distance <= 2^w - 262, the allowed echo taken at exactly its distance,
    lengths, block sizes, BFINAL and the closing stored block; the random bytes stored 65535 to a block; zlib inflates every
    entry, and the device's own decoder every final one, to the same length and CRC."""
    noise = synth.incompressible_cases()
    for k, w in enumerate(windows):
        cases = synth.echo_cases(w)
        names = [c[0] for c in cases] + [c[0] for c in noise]
        datas = [c[1] for c in cases] + [c[1] for c in noise]
        periods = [c[2] for c in cases] + [None] * len(noise)
        final = [(i + k + 1) & 1 for i in range(len(datas))]
        zs, crc, status = _deflate_level(gpu, datas, final, level, w)
        for i, d in enumerate(datas):
            where = (level, w, names[i], final[i])
            assert status[i] == 0 and crc[i] == zlib.crc32(d), (where, int(status[i]))
            assert len(zs[i]) <= len(d) + len(d) // 8 + 64, where
            wk = deflate_tokens.check_encoded(zs[i], d, w, final[i], period=periods[i], where=where)
            if i >= len(cases):
                assert len(wk.matches) == 0, where
                deflate_tokens.check_stored_layout(wk, len(d), final[i], where=where)
            assert zlib.decompressobj(-15).decompress(zs[i]) == d, where
        fin = [i for i in range(len(datas)) if final[i]]
        b = gpu.make_batch([zs[i] for i in fin], [len(datas[i]) + 8 for i in fin])
        out_len, in_used, crc2, st2 = gpu.run_inflate(b)
        assert (st2 == 0).all() and (crc2 == crc[fin]).all(), (level, w)
        assert (out_len == np.array([len(datas[i]) for i in fin])).all() and (in_used == np.array([len(zs[i]) for i in fin])).all(), (level, w)


def _segments(w):
    """[(name, data, period, where the second copy starts)]: segments of several pieces (the WRITE paths cut 16 KiB pieces, 8 KiB
    for a short stream at a low level, and hand each the 32 KiB in front).  The echoes are placed so that R's first copy ends
    where a piece ends and its second copy opens the next piece: every match at the echo's distance starts in the history.
    One echo at the largest distance the window allows, one at 2^w, which it does not."""
    text, _ = synth.bench_corpus()
    out = [("text_echo", (text * (3 * (1 << w) // len(text) + 1))[:3 * (1 << w)], None, 0)]
    for p in ((1 << w) - 262, 1 << w):
        pad = -p % 16384
        r = np.random.RandomState(50 * w + (p & 1)).bytes(p)
        out.append(("echo/%d across a cut" % p, text[1000:1000 + pad] + r + r + r[:300] + text[:5000], p, pad + p))
    return out


def test_host_segment_window_bound(gpu):
    """mzhip_deflate_host_a (what mz_stream_zlib WRITE calls per segment): the segment's pieces, read as ONE stream, keep every
    distance within 2^w - 262 across the cuts between them -- the matches into a piece's history included, which the allowed
    echo must use -- end as the caller asked (final or not), and *crc / *adler are zlib's of the segment."""
    mz = gpu.mz
    L = mz.lib()
    for w in (9, 12, 15):
        for name, d, period, second in _segments(w):
            a = np.frombuffer(d, dtype=np.uint8).copy()
            for level in (1, 6, 9):
                for final in (0, 1):
                    cap = len(d) + len(d) // 8 + 64 * (len(d) // 8192 + 2)      # (every piece may take its own + 64)
                    out = np.zeros(cap, dtype=np.uint8)
                    ol, crc, adler = C.c_uint32(), C.c_uint32(), C.c_uint32()
                    args = mz.DeflateHostArgs(size=C.sizeof(mz.DeflateHostArgs), in_len=len(d), final=final, out_cap=cap, level=level,
                                              window_log2=w, in_=a.ctypes.data, out=out.ctypes.data, out_len=C.addressof(ol),
                                              crc=C.addressof(crc), adler=C.addressof(adler))
                    where = (w, name, level, final)
                    assert L.mzhip_deflate_host_a(C.byref(args)) == 0, where
                    assert crc.value == zlib.crc32(d) and adler.value == zlib.adler32(d), where
                    z = out[:ol.value].tobytes()
                    wk = deflate_tokens.check_encoded(z, d, w, final, period=period if period is not None and period <= (1 << w) - 262 else None,
                                                      where=where, pieces=True)
                    assert sum(1 for b in wk.blocks if b.btype == 0 and b.out_end == b.out_start) >= len(d) // 16384 - (1 if final else 0), where
                    if period is not None and period <= (1 << w) - 262:
                        m = wk.matches
                        assert ((m[:, 2] == period) & (m[:, 0] >= second)).any(), (where, "the echo across the cut is not taken")
                    assert zlib.decompressobj(-15).decompress(z) == d, where


def test_stream_write_window_bound(gpu):
    """The drop-in mz_stream_zlib WRITE with a raw window of -9 / -12 / -15 (COMPRESS_WINDOW): the whole stream -- segments,
    pieces, whatever the shim makes of the writes -- keeps the window it was opened with; the reference, opened with the same
    window, reads it back where it is there."""
    if not os.path.exists(DROP):
        pytest.skip("integration/_build/libmzhipdrop.so missing (it is built from the reference tree)")
    hip = oracle.MzDriver(DROP)
    ref = oracle.ref() if oracle.have_ref() else None
    text, _ = synth.bench_corpus()
    for w in (9, 12, 15):
        n = 3 * (1 << w) + 70000
        d = (text * (n // len(text) + 1))[:n]
        for level in (1, 6, 9):
            z, info = hip.stream_encode(8, d, level=level, window_bits=-w)
            where = (w, level)
            assert (info["open"], info["error"], info["close"], info["total_in"], info["total_out"]) == (0, 0, 0, len(d), len(z)), where
            deflate_tokens.check_encoded(z, d, w, 1, where=where, pieces=True)
            if ref is not None:
                r = ref.stream_decode(8, z, len(d) + 64, window_bits=-w)
                assert (r["out"], r["error"], r["total_in"]) == (d, 0, len(z)), where
