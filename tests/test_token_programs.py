"""CPU tests of the token programs (tests/token_programs.py): the writer against zlib and the token walker, the programs
through the 64-lane emulation of the device code -- the default build and the builds of test_kernel_emul.emu_staged --, the
counters that show every family reaches the mechanism it aims at, and the many-wave window through the host mock."""
import ctypes as C
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import oracle
from tests import token_programs as T
from tests.deflate_tokens import DeflateError, walk
from tests.test_kernel_emul import ROOT, _build_variant, _run, emu, emu_staged  # noqa: F401  (the fixtures, built the same way)


def _zlib(z, zdict=None):
    """-> (bytes, unused input) of zlib's raw inflate, None when it refuses z or does not see its end"""
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    try:
        out = d.decompress(z)
    except zlib.error:
        return None
    return (out, d.unused_data) if d.eof else None


def test_writer_against_zlib_and_the_walker():
    """Nothing else here may be believed until this passes: for every program of every family zlib's raw inflate returns
    exactly expand(program) and consumes exactly the stream; it refuses exactly the programs for which expand() is None; and
    the token walker reads back the tokens that were written -- positions, lengths, distances, block types, BFINAL."""
    n = 0
    for fam in T.FAMILIES:
        entries = T.family(fam)
        assert len({e[0] for e in entries}) == len(entries), fam
        for name, prog, z, data in entries:
            assert data is not None, name
            got = _zlib(z + b"\x5a")                       # (a byte behind the stream: zlib must leave exactly it)
            assert got is not None and got[0] == data and got[1] == b"\x5a", name
            w = walk(z, data=True)
            matches, blocks = T.tokens_of(prog)
            assert w.data == data and (w.bits + 7) // 8 == len(z), name
            assert w.matches.tolist() == [list(m) for m in matches], name
            assert [(b.btype, b.bfinal, b.out_end - b.out_start) for b in w.blocks] == blocks, name
            n += 1
    assert n >= 1800, n
    bad = T.refused()
    for name, prog, z in bad:
        assert T.expand(prog) is None and _zlib(z) is None, name
        with pytest.raises(DeflateError, match="in front of the first byte"):
            walk(z)
    assert len(bad) >= 300
    for name, prog, hist in T.window_programs():
        z = T.encode(prog)
        data = T.expand(prog, hist)
        if data is None:
            assert _zlib(z, hist) is None and name.endswith("too_far"), name
            assert T.expand(prog[:5], hist) is not None and T.expand(prog[:6], hist) is None, name    # (block 5 holds the bad distance)
        else:
            assert _zlib(z, hist) == (data, b""), name
            assert [b.btype for b in walk(z, history=len(hist)).blocks] == [k[0] for k in T.tokens_of(prog)[1]], name


def test_code_shapes_are_complete_and_as_named():
    """code_lengths(): every shape is complete by Kraft's sum, flat gives the used symbols one length, skew1 one bit to the
    chosen symbol, deep 15 bits to some used symbol; headers sent with the repeat codes decode to the same block."""
    rnd = random.Random(5)
    for n in (1, 2, 3, 5, 16, 17, 100, 256, 257, 280, 286):
        freq = {s: 1 + rnd.randrange(1000) for s in rnd.sample(range(286), n)}
        for shape in ("flat", "skew1", "deep", "huff"):
            lens = T.code_lengths(freq, shape)
            assert sum((1 << 15) >> l for l in lens if l) == 1 << 15 and max(lens) <= 15 and all(lens[s] for s in freq), (n, shape)
            used = {lens[s] for s in freq}
            if shape == "flat" and n <= 256:
                assert len(used) == 1, (n, used)
            if shape == "skew1" and n <= 256:
                assert lens[max(freq, key=lambda s: (freq[s], -s))] == 1
            if shape == "deep" and n <= 256:
                assert 15 in used
    assert T.code_lengths({}, "flat", 30, single_ok=True) == [0] * 30
    assert sorted(T.code_lengths({7: 3}, "huff", 30, single_ok=True)) == [0] * 29 + [1]
    toks = [rnd.randrange(256) for _ in range(300)] + [(258, 300), (3, 1), (40, 7)]
    for shape in ("flat", "skew1", "deep", "huff"):
        a = T.encode([("dynamic", toks, True, {"shape": shape})])
        b = T.encode([("dynamic", toks, True, {"shape": shape, "rle": True})])
        assert len(b) < len(a) and _zlib(a) == _zlib(b) == (T.expand([("dynamic", toks, True)]), b""), shape


def _check(fn, tag, name, z, data, it):
    st, used, out, crc = _run(fn, z, len(data) + (it % 3), mis=it % 4, omis=(it // 4) % 4)
    assert st == 0, (tag, name, st)
    assert used == len(z) and len(out) == len(data) and crc == zlib.crc32(data), (tag, name, used, len(z), len(out), len(data))
    assert out == data, (tag, name, "first wrong byte at %d" % next(i for i in range(len(data)) if out[i] != data[i]))


def test_emulation_decodes_every_program(emu, emu_staged):
    """Every accepted program through emul_inflate (span path) and emul_inflate_steps (step loop alone), input and output
    misaligned by 0 .. 3 bytes in turn: status, bytes, consumed input and CRC-32 against zlib's.  Every program on the
    default build, on c_caps and on c_pool; a seeded third of them on c_short and c_serial_cl (the full cross product of
    1 900 programs, two front ends and five builds takes minutes on one core).  Refused programs: the status of the oracle
    restatement (-3), and -200 for an out_cap one byte short."""
    caps, short_, pool, serial = emu_staged
    rnd = random.Random(1)
    it = n_third = 0
    for name, prog, z, data in T.all_accepted():
        builds = [("default", emu), ("c_caps", caps), ("c_pool", pool)]
        if rnd.randrange(3) == 0:
            builds += [("c_short", short_), ("c_serial_cl", serial)]
            n_third += 1
        for tag, L in builds:
            _check(L.emul_inflate, tag, name, z, data, it)
            if len(data) <= (256 << 10) or tag == "default":        # (the step loop alone takes a second per MiB of run)
                _check(L.emul_inflate_steps, tag + "/steps", name, z, data, it + 1)
        it += 1
    assert it >= 1800 and n_third >= 500, (it, n_third)
    n_bad = 0
    for name, prog, z in T.refused():
        want = oracle.inflate_raw(z, 70000)[0]
        assert want == -3, name
        for tag, L in (("default", emu), ("c_caps", caps), ("c_pool", pool)):
            for fn in (L.emul_inflate, L.emul_inflate_steps):
                assert _run(fn, z, 70000, mis=n_bad % 4, omis=(n_bad // 4) % 4)[0] == want, (tag, name)
        n_bad += 1
    assert n_bad >= 300
    for name, prog, z, data in T.family("flood"):
        assert oracle.inflate_raw(z, len(data) - 1)[0] == -200, name
        for tag, L in (("default", emu), ("c_caps", caps), ("c_pool", pool)):
            for fn in (L.emul_inflate, L.emul_inflate_steps):
                assert _run(fn, z, len(data) - 1)[0] == -200, (tag, name)


# counters of an MZ_STATS build (inflate_core.h MZ_STAT): 10 chunk bytes, 12 list entries, 13 near pieces, 14 near rounds,
# 15 chunks, 21 pieces split between far and near, 22 the "cannot happen" branch of the near copies, 23 windows whose
# chain ran into a record cap (the span limit halves), 24 the most rounds one batch of 64 near pieces took
_STAT = dict(chunk_bytes=10, entries=12, near=13, rounds=14, chunks=15, split=21, cannot=22, capped=23, max_rounds=24)


@pytest.fixture(scope="module")
def emu_stats():
    L = _build_variant("stats", ["-DMZ_STATS"])
    L.emul_stats.restype = C.POINTER(C.c_ulonglong)
    return L


def _stats_of(L, z, data):
    s = L.emul_stats()
    for i in range(32):
        s[i] = 0
    st, used, out, crc = _run(L.emul_inflate, z, len(data))
    assert (st, used, out) == (0, len(z), data)
    return {k: int(s[i]) for k, i in _STAT.items()}


def test_programs_reach_what_they_aim_at(emu_stats):
    """The counters of the emulation, per family: chains need a batch of 64 near pieces to take 32 rounds or more; their
    no-dependency form has near pieces and no batch of more than 2 rounds; straddle splits pieces between far and near;
    flood (a) runs into the record cap; flood (b) cuts its chunks at the 4096-byte limit; and no program of any family
    reaches the branch marked "cannot happen".  Measured on the default build: chains up to 64 rounds in a batch (every
    piece waits for the one before), the no-dependency form 1 round; straddle 1 to 4 split pieces per "creep" program and
    up to 7 per fixed-distance program, none in "grow" (its source never moves: near in the first chunk, far in all others);
    flood (a) 3 capped windows; flood (b) with 255-byte matches 3984 bytes per chunk (4080 but for the first and the last),
    with 258-byte matches 2068 (a lane's eight records are 2064 bytes, two lanes are 32 too many); "cannot happen" 0."""
    seen = {}
    for fam in T.FAMILIES:
        for name, prog, z, data in T.family(fam):
            seen[name] = s = _stats_of(emu_stats, z, data)
            assert s["cannot"] == 0, name
    for k in sorted(_STAT):
        print("counter %-11s" % k, {f: max(v[k] for n, v in seen.items() if n.startswith(f + "/")) for f in T.FAMILIES})
    chains = {n: v for n, v in seen.items() if n.startswith("chains/") and "/nodep/" not in n}
    nodep = {n: v for n, v in seen.items() if n.startswith("chains/nodep/")}
    assert max(v["max_rounds"] for v in chains.values()) >= 32
    assert sum(v["max_rounds"] >= 32 for v in chains.values()) >= 20           # (not one lucky program)
    assert nodep and all(v["near"] > 0 and v["max_rounds"] <= 2 for v in nodep.values()), nodep
    straddle = {n: v for n, v in seen.items() if n.startswith("straddle/")}
    assert all(v["split"] > 0 for n, v in straddle.items() if "/creep/" in n), {n: v["split"] for n, v in straddle.items()}
    assert sum(v["split"] > 0 for v in straddle.values()) >= 40
    assert seen["flood/a/skew1"]["capped"] >= 2 and seen["flood/a/deep"]["capped"] >= 2
    for name in ("flood/b/len255/dist1", "flood/b/len255/dist258"):
        s = seen[name]
        assert s["chunks"] >= 100 and s["chunk_bytes"] / s["chunks"] >= 3900, (name, s)    # (16 matches of 255 bytes: 4080; 17 do not fit 4096)
    assert max(v["split"] for n, v in seen.items() if n.startswith("periods/")) > 0
    assert max(v["max_rounds"] for n, v in seen.items() if n.startswith("mix/")) >= 8


MOCK = os.path.join(ROOT, "tests", "emul", "_build", "libmockdrop.so")
def test_many_wave_window_on_the_mock():
    """The multi-block programs of tests/test_gpu_token_programs.py through the host mock's mzhip_inflate_parallel_host (the
    product's inflate_parallel.inc over the emulated device functions): source-map chains a million links deep, blocks that
    read only the block before, chains and straddles cut into blocks, empty blocks between them, history in front of the
    buffer reached to its first byte and one byte beyond."""
    if os.path.isdir("/root/reference"):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True, capture_output=True)
    if not os.path.exists(MOCK):
        pytest.skip("tests/emul/_build/libmockdrop.so needs the reference sources at build time")
    L = C.CDLL(MOCK)
    assert hasattr(L, "mzhip_inflate_parallel_host") and hasattr(L, "mzhip_inflate_host_a")
    progs = T.window_programs()
    assert 10 <= len(progs) <= 40
    nblk = nbytes = 0
    for name, prog, hist in progs:
        assert 4 <= len(prog) <= 200 and all(b[0] != "fixed" for b in prog), name
        b, n = T.run_window_program(L, name, prog, hist)
        nblk += b
        nbytes += n
    print("many-wave window on the mock: %d programs, %d blocks, %d bytes" % (len(progs), nblk, nbytes))
    assert nblk >= 300
