"""The bounds checker of the GPU tests (tests/gpu_util.check_guards) on CPU tensors, no kernel involved: it must see each of
the stores it exists for -- and name the entry -- and pass a batch that a well-behaved "kernel" filled in."""
import numpy as np
import pytest

from tests import gpu_util

LAYOUTS = [dict(guard=67, align=1, odd=True), dict(guard=64, packed=True), dict(guard=32, align=16)]


def _filled(layout, n=9):
    """a batch as a correct launch leaves it: entry i holds out_len[i] bytes of value 0 (never in the pattern), its result
    words are written, everything else is untouched"""
    import torch

    rnd = np.random.RandomState(5)
    caps = [int(c) for c in rnd.randint(0, 400, size=n)]
    caps[3] = 0
    pays = [rnd.bytes(int(k)) for k in rnd.randint(0, 90, size=n)]
    b = gpu_util.make_batch(pays, caps, device="cpu", fill=11, **layout)
    out_len = np.array([c - (i % 3) * (c > 3) for i, c in enumerate(caps)], dtype=np.int64)
    status = np.zeros(n, dtype=np.int32)
    status[5] = -3
    res = gpu_util.guarded_results(n, ("out_len", "status", "crc", "state"), words={"state": 4}, device="cpu")
    h = b["d_out"].numpy()
    for i in range(n):
        o = int(b["h_out_off"][i])
        h[o:o + int(out_len[i])] = 0
    h[int(b["h_out_off"][5]) + caps[5] - 1] = 0          # a failing entry may have used its whole region
    res["out_len"][:n] = torch.from_numpy(out_len.astype(np.int32))
    res["status"][:n] = torch.from_numpy(status)
    res["crc"][:n] = 7
    res["state"][:4 * n] = 1
    return b, out_len, status, res, caps


def _check(b, out_len, status, res):
    return gpu_util.check_guards(b, out_len, status, results=res, words={"state": 4})


@pytest.mark.parametrize("layout", LAYOUTS)
def test_untouched_batch_passes(layout):
    b, out_len, status, res, caps = _filled(layout)
    assert (b["h_fill"] != 0).all() and len(set(b["h_fill"][:64].tolist())) > 8          # the pattern: never zero, not constant
    assert (b["d_out"].numpy()[:b["guard"]] == b["h_fill"][:b["guard"]]).all()
    off = b["h_out_off"]
    if layout.get("packed"):
        assert all(off[i + 1] == off[i] + caps[i] for i in range(len(caps) - 1)) and off[0] == 64
    if layout.get("odd"):
        assert all(int(o) & 1 for o in off)
    _check(b, out_len, status, res)
    # the default layout is the one the suite has always used: zeros, 16-byte alignment, no red zones
    d = gpu_util.make_batch([b"abc", b"", b"x" * 40], [5, 0, 33], device="cpu")
    assert d["h_out_off"].tolist() == [0, 16, 16] and d["d_out"].numel() == 64 and not d["d_out"].any()
    assert d["in_off"].tolist() == [0, 16, 16] and d["d_in"].numel() == 64


@pytest.mark.parametrize("layout", LAYOUTS)
def test_each_stray_store_is_caught_with_its_entry(layout):
    packed = bool(layout.get("packed"))
    # one byte at cap of the LAST entry (in the packed layout only that one has a red zone behind it; a write at cap of any
    # other entry lands in its neighbour's region, which the byte comparison of the neighbour sees)
    b, out_len, status, res, caps = _filled(layout)
    i = len(caps) - 1
    b["d_out"][int(b["h_out_off"][i]) + caps[i]] = 0
    with pytest.raises(AssertionError, match=r"\(a\) entry %d: byte at offset %d " % (i, caps[i])):
        _check(b, out_len, status, res)
    if not packed:
        b, out_len, status, res, caps = _filled(layout)
        b["d_out"][int(b["h_out_off"][2]) + caps[2]] ^= 0x80
        with pytest.raises(AssertionError, match=r"\(a\) entry 2: byte at offset %d " % caps[2]):
            _check(b, out_len, status, res)
    # one byte in front of out_off
    b, out_len, status, res, caps = _filled(layout)
    b["d_out"][int(b["h_out_off"][0]) - 1] = 0
    with pytest.raises(AssertionError, match=r"\(a\) byte \d+ of d_out, 1 in front of entry 0"):
        _check(b, out_len, status, res)
    if not packed:
        b, out_len, status, res, caps = _filled(layout)
        b["d_out"][int(b["h_out_off"][4]) - 1] = 0
        with pytest.raises(AssertionError, match=r"\(a\) entry 3: .*next entry 4 starts"):
            _check(b, out_len, status, res)
    # a changed input byte
    b, out_len, status, res, caps = _filled(layout)
    k = next(i for i in range(len(caps)) if int(b["h_in_len"][i]) > 2)
    b["d_in"][int(b["h_in_off"][k]) + 2] ^= 1
    with pytest.raises(AssertionError, match=r"\(b\) entry %d: input byte at offset 2 " % k):
        _check(b, out_len, status, res)
    # a store to result element n (and to word 0 of state n)
    for name, w in (("status", 1), ("crc", 1), ("state", 4)):
        b, out_len, status, res, caps = _filled(layout)
        res[name][len(caps) * w] = 0
        with pytest.raises(AssertionError, match=r"\(c\) result array '%s': element %d \(entry %d" % (name, len(caps) * w, len(caps))):
            _check(b, out_len, status, res)
    # a result word that was never written
    b, out_len, status, res, caps = _filled(layout)
    res["status"][6] = int(np.array([gpu_util.SENTINEL], dtype=np.uint32).view(np.int32)[0])
    with pytest.raises(AssertionError, match=r"\(c\) result array 'status': entry 6 of"):
        _check(b, out_len, status, res)
    # a write at out_len of a status-0 entry
    b, out_len, status, res, caps = _filled(layout)
    k = next(i for i in range(len(caps)) if out_len[i] < caps[i] and status[i] == 0)
    b["d_out"][int(b["h_out_off"][k]) + int(out_len[k])] = 0
    with pytest.raises(AssertionError, match=r"\(d\) entry %d \(status 0, out_len %d" % (k, out_len[k])):
        _check(b, out_len, status, res)
    gpu_util.check_guards(b, out_len, status, results=res, words={"state": 4}, slack_ok=True)      # the per-kernel flag
    # ... of a failing entry: its own region is its own
    b, out_len, status, res, caps = _filled(layout)
    b["d_out"][int(b["h_out_off"][5]) + int(out_len[5])] = 0
    _check(b, out_len, status, res)
    # checksum launches own no output at all
    b, out_len, status, res, caps = _filled(layout)
    with pytest.raises(AssertionError, match=r"\(a\) "):
        gpu_util.check_guards(b, out_len, status, outputs=False)
