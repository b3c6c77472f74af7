"""GPU tests of the token programs (tests/token_programs.py): DEFLATE streams written token by token -- period copies at
every alignment, chains of matches that read each other, sources that straddle a chunk's start, codes skewed until a span
overruns the record caps, trains of tiny blocks, distances that reach byte 0 and one byte further -- through
mzhip_inflate_batch and, block by block on waves of their own, through mzhip_inflate_parallel_host.  zlib's inflate is the
judge (tests/test_token_programs.py holds the writer against it on the CPU).

Caps of this file: at most 4096 entries and 32 MiB of expected output per launch, no entry above 1 MiB."""
import random
import zlib

import numpy as np
import pytest

import oracle
from tests import token_programs as T

pytestmark = pytest.mark.gpu

MAX_ENTRIES, MAX_LAUNCH_BYTES, MAX_ENTRY_BYTES = 4096, 32 << 20, 1 << 20


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util

    gpu_util.mz.require_gpu()
    return gpu_util


def _launch(gpu, entries, caps, **layout):
    """entries: [(name, stream, bytes or None)] -> per-entry results of ONE mzhip_inflate_batch launch and the output buffer"""
    assert len(entries) <= MAX_ENTRIES and sum(len(e[2]) for e in entries if e[2]) <= MAX_LAUNCH_BYTES
    batch = gpu.make_batch([e[1] for e in entries], caps, **layout)
    out_len, in_used, crc, status = gpu.run_inflate(batch)
    return batch, batch["d_out"].cpu().numpy(), out_len, in_used, crc, status


def _check_good(gpu, what, batch, h_out, res, i, name, z, data):
    out_len, in_used, crc, status = res
    assert status[i] == 0, (what, name, int(status[i]))
    assert out_len[i] == len(data) and in_used[i] == len(z), (what, name, int(out_len[i]), len(data), int(in_used[i]), len(z))
    got = gpu.entry_bytes(batch, h_out, i, len(data))
    if got != data:
        bad = next(k for k in range(len(data)) if got[k] != data[k])
        raise AssertionError("%s: %s: byte %d of %d is %d, zlib says %d" % (what, name, bad, len(data), got[bad], data[bad]))
    assert int(crc[i]) == zlib.crc32(data), (what, name)


def test_batch_token_programs(gpu):
    """Every accepted program of every family in ONE launch, entries laid out byte by byte (align=1); once more packed, so
    that the output misalignment of an entry takes every value; once more in a seeded shuffled order: results are per entry
    and do not depend on the neighbours.  out_cap is the exact size for every second entry, 1 .. 64 bytes more for the rest.
    Per entry: status 0, out_len, in_used == len(stream), the bytes and the CRC-32 against zlib's."""
    entries = [(n, z, d) for n, p, z, d in T.all_accepted()]
    total = sum(len(d) for _, _, d in entries)
    print("test_batch_token_programs: %d entries, %d bytes of expected output per launch, largest entry %d"
          % (len(entries), total, max(len(d) for _, _, d in entries)))
    assert 1800 <= len(entries) <= MAX_ENTRIES and total <= MAX_LAUNCH_BYTES and max(len(d) for _, _, d in entries) <= MAX_ENTRY_BYTES
    for fam in T.FAMILIES:
        assert T.family(fam), fam
    caps = [len(d) + (0 if i % 2 == 0 else 1 + (i * 7) % 64) for i, (_, _, d) in enumerate(entries)]
    order = list(range(len(entries)))
    random.Random(20).shuffle(order)
    for what, idx, layout in (("align=1", None, dict(align=1)), ("packed", None, dict(packed=True, odd=True)), ("shuffled", order, dict(align=1))):
        es = entries if idx is None else [entries[k] for k in idx]
        cs = caps if idx is None else [caps[k] for k in idx]
        batch, h_out, *res = _launch(gpu, es, cs, **layout)
        if what == "packed":
            assert len({int(o) & 15 for o in batch["h_out_off"]}) == 16          # every misalignment of out + out_pos
        for i, (name, z, data) in enumerate(es):
            _check_good(gpu, what, batch, h_out, res, i, name, z, data)


def test_batch_token_programs_refused(gpu):
    """The refused twins of the edges family (a distance one byte too far: first token, behind 10 tokens, behind 5000 tokens
    deep in a span among far pieces, in the last 30 bytes) and the flood programs with out_cap one byte short, one bad entry
    to three good ones in one launch.  The verdicts are the oracle restatement's, -3 and -200; every good neighbour is exact."""
    bad = [(n, z, None, 70000, -3) for n, p, z in T.refused()]
    bad += [(n + "/cap-1", z, None, len(d) - 1, -200) for n, p, z, d in T.family("flood")]
    good = [(n, z, d) for n, p, z, d in T.all_accepted() if len(d) <= (64 << 10)]
    random.Random(21).shuffle(good)
    entries, caps, want = [], [], []
    for i, (n, z, _, cap, st) in enumerate(bad):
        assert oracle.inflate_raw(z, cap)[0] == st, n
        entries.append((n, z, None))
        caps.append(cap)
        want.append(st)
        for n2, z2, d2 in good[3 * i:3 * i + 3]:
            entries.append((n2, z2, d2))
            caps.append(len(d2) + i % 2)
            want.append(0)
    n_good = sum(w == 0 for w in want)
    print("test_batch_token_programs_refused: %d entries (%d refused, %d good), %d bytes of expected output"
          % (len(entries), len(bad), n_good, sum(len(e[2]) for e in entries if e[2])))
    assert len(bad) >= 320 and n_good == 3 * len(bad) and len(entries) <= MAX_ENTRIES
    batch, h_out, *res = _launch(gpu, entries, caps, align=1)
    for i, (name, z, data) in enumerate(entries):
        if want[i]:
            assert res[3][i] == want[i], (name, int(res[3][i]), want[i])
        else:
            _check_good(gpu, "refused neighbours", batch, h_out, res, i, name, z, data)


def test_many_wave_window_token_programs(gpu):
    """Programs of 4 to 200 dynamic and stored blocks through mzhip_inflate_parallel_host, one call each: a distance-1 run of
    1 MiB over 50 blocks (source-map chains a million links deep), blocks that read only the block before them, chains and
    straddles cut into blocks, end-of-block-only blocks between them, and history of 1, 100 and 32768 bytes in front of the
    buffer with matches that reach its first byte -- or one byte further, which must end the chain in front of that block.
    What the call declines is finished by mzhip_inflate_host_a from the state handed back (T.run_window_program asserts
    rc, bytes, checksums, block count, state against zlib)."""
    L = gpu.mz.lib()
    progs = T.window_programs()
    assert 10 <= len(progs) <= 40
    nblk = nbytes = n4 = 0
    for name, prog, hist in progs:
        assert 4 <= len(prog) <= 200 and all(b[0] != "fixed" for b in prog), name
        b, n = T.run_window_program(L, name, prog, hist)
        assert n <= MAX_ENTRY_BYTES
        nblk += b
        nbytes += n
        n4 += b >= 4
    print("test_many_wave_window_token_programs: %d windows, %d blocks decoded by waves of their own, %d bytes of expected output"
          % (len(progs), nblk, nbytes))
    assert n4 >= 20 and nblk >= 450 and nbytes <= MAX_LAUNCH_BYTES
