"""GPU tests of the far and near lists of K1's commit (inflate_emit.inc, inflate_commit.inc) on the entries of
tests/far_near_cases.py -- the CPU twin on the host emulation, with the kernel's counters, is tests/test_far_near_lists_emul.py --
through mzhip_inflate_batch: one launch per group of at most 64 entries, each at most 64 KiB.  zlib judges the bytes; out_len,
in_used, CRC-32 and status must also be what the host emulation of the same sources answers.  Then 256 level-6 and 256 level-1
slices of the bench corpus of 8 KiB and of 64 KiB, against zlib.  No timing."""
import random
import zlib

import pytest

from tests import far_near_cases as FN
from tests import synth

pytestmark = pytest.mark.gpu

GROUP = 64


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


def _launch(gpu, streams, caps, **layout):
    assert len(streams) <= GROUP and max(caps) <= 65536 + 64
    batch = gpu.make_batch(streams, caps, **layout)
    out_len, in_used, crc, status = gpu.run_inflate(batch)
    return batch, batch["d_out"].cpu().numpy(), out_len, in_used, crc, status


def test_far_near_cases(gpu):
    """every case byte for byte against zlib and word for word against the emulation, laid out byte by byte (every entry at
    another 16-byte misalignment) and once more with red zones between the entries"""
    cases = FN.accepted() + FN.refused()
    emul = [FN.decode(c["z"], c["cap"])[0] for c in cases]
    for c, words in zip(cases, emul):
        if c in FN.refused():
            assert words == FN.REFUSED_PARENT
        else:
            assert words == (0, len(c["data"]), len(c["z"]), zlib.crc32(c["data"])), c["name"]
    for layout in (dict(align=1), dict(guard=64, fill=5)):
        for g in range(0, len(cases), GROUP):
            group = cases[g:g + GROUP]
            batch, h_out, out_len, in_used, crc, status = _launch(gpu, [c["z"] for c in group], [c["cap"] for c in group], **layout)
            for i, c in enumerate(group):
                st, ol, iu, cr = emul[g + i]
                assert (int(status[i]), int(out_len[i]), int(in_used[i])) == (st, ol, iu), (c["name"], layout, int(status[i]), int(out_len[i]), int(in_used[i]))
                got = gpu.entry_bytes(batch, h_out, i, ol)
                if got != c["data"][:ol]:
                    bad = next(k for k in range(ol) if got[k] != c["data"][k])
                    raise AssertionError("%s: byte %d of %d is %d, zlib says %d" % (c["name"], bad, ol, got[bad], c["data"][bad]))
                if st == 0:
                    assert int(crc[i]) == cr == zlib.crc32(c["data"]), c["name"]
            if "guard" in layout:
                gpu.check_guards(batch, out_len, status)


@pytest.mark.parametrize("size", [8192, 65536])
def test_corpus_slices(gpu, size):
    """256 slices at level 6 and 256 at level 1, 64 entries a launch"""
    text = synth.bench_corpus()[0]
    rnd = random.Random(size)
    for level in (6, 1):
        datas = [bytes(text[o:o + size]) for o in (rnd.randrange(len(text) - size) for _ in range(256))]
        pays = [synth.deflate_raw(d, level) for d in datas]
        for g in range(0, 256, GROUP):
            batch, h_out, out_len, in_used, crc, status = _launch(gpu, pays[g:g + GROUP], [size] * GROUP, packed=True)
            for i in range(GROUP):
                d = datas[g + i]
                assert (int(status[i]), int(out_len[i]), int(in_used[i])) == (0, size, len(pays[g + i])), (level, g + i)
                assert gpu.entry_bytes(batch, h_out, i, size) == d and int(crc[i]) == zlib.crc32(d), (level, g + i)
