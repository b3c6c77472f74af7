"""Wave reuse: an entry comes out the same behind any other entry.

Every batch kernel is a grid of persistent waves; a wave takes an entry index from a counter, codes the entry and takes the
next with the same LDS slice and the same scratch in HBM.  The other GPU tests either stay under the resident grid (every
wave codes one entry) or cross it with entries of one sort.  Here every launch has n = max(4 W, 64 CU) + 5 entries (W = the
waves of K1's full grid, CU = the compute units): no kernel holds more than 32 waves per CU, so every resident wave of every
kernel takes two entries at least, K1's about four -- by counting alone, no launcher constant is read.  The entries are the
kinds of synth.reuse_kinds() (tests/test_kernel_emul.py runs the same table in ordered pairs through the CPU emulation):
"phased" = the first 32 CU indices are refused kinds only and the rest good ones, so a wave that took one of the first
decodes a good entry straight behind a refused one; "shuffled" = a seeded permutation of all kinds.  Both in the two layouts
of test_gpu_bounds, over a seeded byte pattern: the whole of d_out is compared with a blob built on the host."""
import time
import zlib

import numpy as np
import pytest

from tests import synth
from tests.test_gpu_bounds import (LAYOUTS, _geometry, _got, _unwrap_lzma, launch_deflate, launch_inflate, launch_lzma,
                                   launch_lzma_encode)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


def _size(gpu):
    """-> (n, W, CU)"""
    import torch

    w = _geometry(gpu) * 4
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = max(4 * w, 64 * cu) + 5
    assert n > 32 * cu
    return n, w, cu


def _goods(kinds, m):
    """m indices of good kinds, in turn; one in 97 a long one"""
    small = [i for i, kd in enumerate(kinds) if kd["refused"] is None and not kd["long"]]
    longs = [i for i, kd in enumerate(kinds) if kd["long"]]
    return [longs[(j // 97) % len(longs)] if longs and j % 97 == 96 else small[j % len(small)] for j in range(m)]


def _orders(kinds, n, cu, seed):
    """(name, kind index of every entry) of the two launches"""
    refused = [i for i, kd in enumerate(kinds) if kd["refused"] is not None]
    phased = [refused[j % len(refused)] for j in range(32 * cu)] + _goods(kinds, n - 32 * cu)
    mixed = [refused[j % len(refused)] for j in range(n // 4)] + _goods(kinds, n - n // 4)
    mixed = [mixed[j] for j in np.random.RandomState(seed).permutation(n)]
    # cap on what is left out of the byte comparison, from the reference alone: two thirds of the shuffled launch decode
    assert 3 * sum(kinds[i]["status"] == 0 for i in mixed) >= 2 * n
    assert all(kinds[i]["status"] != 0 for i in phased[:32 * cu]) and all(kinds[i]["status"] == 0 for i in phased[32 * cu:])
    return (("phased", phased), ("shuffled", mixed))


def _expected(b, kinds, idx):
    """the host's d_out: the reference's bytes in every status-0 entry's region, the pattern everywhere else; and the mask of
    what is not compared: the regions of refused entries, and what lies behind the clamped length of an entry decoded under
    TOTAL_OUT_MAX (include/mzhip.h: the stream is decoded to its end inside out_cap)"""
    exp = b["h_fill"].copy()
    skip = np.zeros(exp.size, dtype=bool)
    data = [np.frombuffer(kd["data"], dtype=np.uint8) for kd in kinds]
    for e, i in enumerate(idx):
        kd = kinds[i]
        o = int(b["h_out_off"][e])
        if kd["status"] != 0:
            skip[o:o + kd["cap"]] = True
            continue
        exp[o:o + kd["out_len"]] = data[i]
        if kd["max_out"] >= 0:
            skip[o + kd["out_len"]:o + kd["cap"]] = True
    return exp, skip


def _compare_blob(gpu, b, h, exp, skip, kinds, idx, what):
    bad = np.flatnonzero((h != exp) & ~skip)
    if bad.size:
        j = int(bad[0])
        e = int(np.searchsorted(b["h_out_off"], j, side="right")) - 1
        raise AssertionError("%s: entry %d (%s; the entry in front: %s): byte %d of its region is %d, expected %d; %d such bytes" % (
            what, e, kinds[idx[e]]["name"], kinds[idx[e - 1]]["name"] if e else "none", j - int(b["h_out_off"][e]), h[j], exp[j], bad.size))


def _fresh_words(gpu, kinds, launch):
    """{kind index: (in_used, out_len, crc)} of every refused kind from a launch of that entry alone (a wave that has coded
    nothing before): what these words hold behind a refusal is not what the oracle restatement holds (it stops elsewhere in the
    stream, and include/mzhip.h promises them for status 0) -- but it is the same behind any other entry"""
    out = {}
    for i, kd in enumerate(kinds):
        if kd["status"] == 0:
            continue
        b = gpu.make_batch([kd["z"]], [kd["cap"]], fill=31, guard=64)
        R = launch(b, [kd])
        assert int(gpu.result_words(R["status"], 1).view(np.int32)[0]) == kd["status"], (kd["name"], "alone")
        out[i] = tuple(int(gpu.result_words(R[k], 1)[0]) for k in ("in_used", "out_len", "crc"))
    return out


def _decoder(gpu, fam, launch, seed):
    kinds = synth.reuse_kinds()[fam]
    n, w, cu = _size(gpu)
    fresh = _fresh_words(gpu, kinds, launch)
    ref = {k: np.array([kd[k] for kd in kinds], dtype=np.int64) for k in ("status", "in_used", "out_len", "crc")}
    for i, v in fresh.items():
        ref["in_used"][i], ref["out_len"][i], ref["crc"][i] = v
    clamp = any(kd["max_out"] >= 0 for kd in kinds)
    for lname, lay in LAYOUTS:
        for oname, idx in _orders(kinds, n, cu, seed):
            t0 = time.time()
            ents = [kinds[i] for i in idx]
            b = gpu.make_batch([kd["z"] for kd in ents], [kd["cap"] for kd in ents], fill=seed, **lay)
            exp, skip = _expected(b, kinds, idx)
            R = launch(b, ents)
            out_len, status = _got(gpu, R, n)
            h = gpu.check_guards(b, out_len, status, results=R, slack_ok=clamp)
            what = (fam, lname, oname)
            _compare_blob(gpu, b, h, exp, skip, kinds, idx, what)
            ix = np.array(idx)
            got = dict(status=status.astype(np.int64), out_len=out_len, in_used=gpu.result_words(R["in_used"], n).astype(np.int64),
                       crc=gpu.result_words(R["crc"], n).astype(np.int64))
            for k in ("status", "in_used", "out_len", "crc"):
                bad = np.flatnonzero(got[k] != ref[k][ix])
                assert bad.size == 0, (what, k, "entry %d (%s; in front: %s): %d, expected %d; %d such entries" % (
                    int(bad[0]), ents[int(bad[0])]["name"], ents[int(bad[0]) - 1]["name"], int(got[k][bad[0]]), int(ref[k][ix][bad[0]]), bad.size))
            ok = int((ref["status"][ix] == 0).sum())
            print("%s %s %s: n %d, W %d, CU %d; %d of %d entries (%.1f %%) compared byte for byte, %.1f MB of d_out, %.1f s"
                  % (fam, lname, oname, n, w, cu, ok, n, 100.0 * ok / n, h.size / 1e6, time.time() - t0))


def test_inflate_batch_wave_reuse(gpu):
    _decoder(gpu, "deflate", lambda b, ents: launch_inflate(gpu, b), 2100)


def test_lzma_batch_wave_reuse(gpu):
    _decoder(gpu, "lzma", lambda b, ents: launch_lzma(gpu, b, [kd["max_out"] for kd in ents]), 2200)


def test_xz_batch_wave_reuse(gpu):
    _decoder(gpu, "xz", lambda b, ents: launch_lzma(gpu, b, [kd["max_out"] for kd in ents], xz=True), 2300)


# ---- mzhip_inflate_resume_batch ----------------------------------------------------------------------------------------

def _walk(gpu, z, data, sizes):
    """the reference walk: the stream window by window (room sizes[k % len] behind at most 32 KiB of history), every window
    a launch of its own -> [(state in, history, cap, status, in_used, out_len, crc, stop state, new bytes)]"""
    import torch

    wins = []
    got, state = bytearray(), (0, 0, 0, 0)
    for k in range(400):
        hist = state[2]
        cap = hist + sizes[k % len(sizes)]
        b = gpu.make_batch([z], [cap], fill=41, guard=64)
        h0 = b["h_fill"].copy()
        o = int(b["h_out_off"][0])
        h0[o:o + hist] = np.frombuffer(bytes(got[len(got) - hist:]), dtype=np.uint8)
        b["d_out"].copy_(torch.from_numpy(h0))
        b["h_fill"] = h0
        res = torch.tensor([state], dtype=torch.int64).to(torch.int32).to(b["d_in"].device)
        R = launch_inflate(gpu, b, resume=res, stop=True)
        out_len, status = _got(gpu, R, 1)
        h = gpu.check_guards(b, out_len, status, results=R, words={"stop": 4})
        stop = tuple(int(v) for v in gpu.result_words(R["stop"], 1, 4)[0])
        st = int(status[0])
        assert st in (0, -200), (k, st)
        valid = int(out_len[0]) if st == 0 else stop[2]
        assert hist <= valid <= cap
        new = h[o + hist:o + valid].tobytes()
        crc = int(gpu.result_words(R["crc"], 1)[0])
        assert crc == zlib.crc32(new), k
        wins.append((state, bytes(got[len(got) - hist:]), cap, st, int(gpu.result_words(R["in_used"], 1)[0]), int(out_len[0]), crc, stop, new))
        got += new
        if st == 0:
            assert bytes(got) == data
            return wins
        assert stop[3] & 1
        state = (stop[0], stop[1], min(len(got), 32768), 1)
    raise AssertionError("no end")


def test_inflate_resume_batch_wave_reuse(gpu):
    """Every entry is one window of one of two streams with its mz_inflate_state (test_inflate_resume_batch_bounds builds them
    so): consecutive indices alternate streams and window sizes.  What a window gives behind any other window -- status,
    counts, CRC, the stop state, every byte of d_out -- is what it gave in the reference walk, a launch of its own, and the
    walk ended with zlib's bytes."""
    import torch

    n, w, cu = _size(gpu)
    c = synth.corpus()
    K = {kd["name"]: kd for kd in synth.reuse_kinds()["deflate"]}
    streams = [(synth.deflate_raw(c[120000:132000], level=9), c[120000:132000]),
               (K["long_codes/geom0.5/l9"]["z"], K["long_codes/geom0.5/l9"]["data"])]
    walks = [_walk(gpu, streams[0][0], streams[0][1], (300, 7, 4096, 1)), _walk(gpu, streams[1][0], streams[1][1], (4096, 1, 300, 7))]
    assert min(len(x) for x in walks) >= 8
    wins = []                                                   # (stream, window) in the order A0, B0, A1, B1, ...
    for k in range(max(len(x) for x in walks)):
        wins += [(s, k % len(walks[s])) for s in (0, 1)]
    for lname, lay in LAYOUTS:
        t0 = time.time()
        ents = [wins[e % len(wins)] for e in range(n)]
        W = [walks[s][k] for s, k in ents]
        b = gpu.make_batch([streams[s][0] for s, _ in ents], [x[2] for x in W], fill=2400, **lay)
        h0 = b["h_fill"].copy()
        exp_parts = []
        for e, x in enumerate(W):
            o = int(b["h_out_off"][e])
            hist = len(x[1])
            if hist:
                h0[o:o + hist] = np.frombuffer(x[1], dtype=np.uint8)
            exp_parts.append((o + hist, x[8]))
        b["d_out"].copy_(torch.from_numpy(h0))
        b["h_fill"] = h0                                        # the history is the caller's: the guards hold it too
        res = torch.tensor([x[0] for x in W], dtype=torch.int64).to(torch.int32).to(b["d_in"].device)
        R = launch_inflate(gpu, b, resume=res, stop=True)
        out_len, status = _got(gpu, R, n)
        stop = gpu.result_words(R["stop"], n, 4).astype(np.int64)
        h = gpu.check_guards(b, out_len, status, results=R, words={"stop": 4})
        exp = h0.copy()
        skip = np.zeros(exp.size, dtype=bool)                   # a window left with OUT_FULL: what lies behind its stop position
        for e, (o, new) in enumerate(exp_parts):
            exp[o:o + len(new)] = np.frombuffer(new, dtype=np.uint8)
            if W[e][3] != 0:
                skip[o + len(new):int(b["h_out_off"][e]) + W[e][2]] = True
        bad = np.flatnonzero((h != exp) & ~skip)
        assert bad.size == 0, (lname, "byte %d of d_out (entry %d)" % (int(bad[0]), int(np.searchsorted(b["h_out_off"], int(bad[0]), side="right")) - 1), bad.size)
        got = dict(status=status.astype(np.int64), in_used=gpu.result_words(R["in_used"], n).astype(np.int64), out_len=out_len,
                   crc=gpu.result_words(R["crc"], n).astype(np.int64))
        for j, k in enumerate(("status", "in_used", "out_len", "crc")):
            want = np.array([x[3 + j] for x in W], dtype=np.int64)
            bad = np.flatnonzero(got[k] != want)
            assert bad.size == 0, (lname, k, int(bad[0]), ents[int(bad[0])], int(got[k][bad[0]]), int(want[bad[0]]), bad.size)
        want = np.array([x[7] for x in W], dtype=np.int64)
        bad = np.flatnonzero((stop != want).any(axis=1))
        assert bad.size == 0, (lname, "stop state", int(bad[0]), ents[int(bad[0])], stop[bad[0]].tolist(), want[bad[0]].tolist(), bad.size)
        print("resume %s: n %d, W %d, CU %d; %d windows of 2 streams, every entry compared byte for byte up to where it stopped, %.1f MB of d_out, %.1f s"
              % (lname, n, w, cu, len(wins), h.size / 1e6, time.time() - t0))


# ---- encoders ----------------------------------------------------------------------------------------------------------

def _encoder(gpu, launch, back, room, seed, what):
    """Every entry round-trips on the host; all entries of one input came out byte-identical, and identical to the same input
    from a one-entry launch made first."""
    inputs = synth.reuse_kinds()["enc"]
    n, w, cu = _size(gpu)
    caps = [len(d) + len(d) // 8 + room for _, d in inputs]
    fresh = []
    for (name, d), cap in zip(inputs, caps):
        b = gpu.make_batch([d], [cap], fill=51, guard=64)
        R = launch(b)
        out_len, status = _got(gpu, R, 1)
        h = gpu.check_guards(b, out_len, status, results=R)
        z = gpu.entry_bytes(b, h, 0, int(out_len[0]))
        assert status[0] == 0 and back(z, len(d)) == d and int(gpu.result_words(R["crc"], 1)[0]) == zlib.crc32(d), (what, name, "alone")
        fresh.append(z)
    small = [i for i, (_, d) in enumerate(inputs) if len(d) <= 4096]
    longs = [i for i, (_, d) in enumerate(inputs) if len(d) > 4096]
    assert len(longs) == 2
    turn = [longs[(j // 97) % 2] if j % 97 == 96 else small[j % len(small)] for j in range(n)]
    mixed = [turn[j] for j in np.random.RandomState(seed).permutation(n)]
    want_crc = np.array([zlib.crc32(d) for _, d in inputs], dtype=np.int64)
    want_len = np.array([len(z) for z in fresh], dtype=np.int64)
    for lname, lay in LAYOUTS:
        for oname, idx in (("in turn", turn), ("shuffled", mixed)):
            t0 = time.time()
            b = gpu.make_batch([inputs[i][1] for i in idx], [caps[i] for i in idx], fill=seed, **lay)
            exp = b["h_fill"].copy()
            for e, i in enumerate(idx):
                o = int(b["h_out_off"][e])
                exp[o:o + len(fresh[i])] = np.frombuffer(fresh[i], dtype=np.uint8)
            R = launch(b)
            out_len, status = _got(gpu, R, n)
            h = gpu.check_guards(b, out_len, status, results=R)
            assert (status == 0).all(), (what, lname, oname, int(np.flatnonzero(status != 0)[0]))
            ix = np.array(idx)
            seen = set()
            for e, i in enumerate(idx):                        # the round trip of every entry (equal bytes are decoded once)
                z = gpu.entry_bytes(b, h, e, int(out_len[e]))
                if z not in seen:
                    assert back(z, len(inputs[i][1])) == inputs[i][1], (what, lname, oname, e, inputs[i][0])
                    seen.add(z)
            bad = np.flatnonzero(h != exp)
            if bad.size:
                e = int(np.searchsorted(b["h_out_off"], int(bad[0]), side="right")) - 1
                raise AssertionError("%s %s %s: entry %d (%s; in front: %s) differs from the same input coded alone at byte %d; %d such bytes"
                                     % (what, lname, oname, e, inputs[idx[e]][0], inputs[idx[e - 1]][0], int(bad[0]) - int(b["h_out_off"][e]), bad.size))
            assert (out_len == want_len[ix]).all() and (gpu.result_words(R["crc"], n).astype(np.int64) == want_crc[ix]).all(), (what, lname, oname)
            print("%s %s %s: n %d, W %d, CU %d; every entry compared byte for byte, %.1f MB of d_out, %.1f s"
                  % (what, lname, oname, n, w, cu, h.size / 1e6, time.time() - t0))


@pytest.mark.parametrize("level", (1, 6, 9))
def test_deflate_batch_level_wave_reuse(gpu, level):
    _encoder(gpu, lambda b: launch_deflate(gpu, b, level=level), lambda z, k: zlib.decompress(z, -15), 64, 2500 + level, "deflate level %d" % level)


@pytest.mark.parametrize("preset", (1, 6))
def test_lzma_encode_batch_preset_wave_reuse(gpu, preset):
    _encoder(gpu, lambda b: launch_lzma_encode(gpu, b, preset=preset), lambda z, k: _unwrap_lzma(z, 0, k), 1024, 2600 + preset,
             "lzma encode preset %d" % preset)
