"""The entries of tests/test_commit_chains_emul.py and tests/test_gpu_commit_chains.py, for three parts of the commit stage
of K1 (inflate_commit.inc): the CRC fold of several super-tiles of a lane together (crc32_core.h, MZ_CRC_CHAINS), the tail of
a near copy (inflate_core.h mz_copy32_seq) and the group of records an emit round loads (inflate_emit.inc).

  sizes()   entries whose output sizes stand on, one before and one behind every multiple of the 4 KiB super-tile up to a
            group of four, and at 32 / 64 KiB -- where the grouped CRC fold takes a group, leaves tiles pending, or has the
            final single-tile drain take them -- as level-6 text, as stored blocks (of 4000 bytes: a fold call at every
            offset inside a tile; and as one block: several groups in one call) and as level 0 followed by level 6.
  tails()   token programs (tests/token_programs.py): every match length 3 .. 40 and 255 .. 258 at every distance of
            {1 .. 9, 15, 16, 17, 31, 32, 33} -- every tail n & 7 of a near copy behind 0 .. 4 body steps, at every period
            of the short-period prologue and at the distances next to 8, 16 and 32 --
              near   behind max(D, k) fresh literals, k = 0 .. 15: the source lies inside the chunk, at every staging
                     misalignment;
              far    the same cases behind 6 KiB of literals: chunks in front of the case's chunk, out_pos != 0, the literals
                     the match reads may lie in the chunk before;
              split  behind 6 KiB of literals a train of the same matches, one to three literals between them, over more than
                     three chunks: wherever a chunk starts, the match there reads across the start (a far part, and a near
                     remainder whose length is whatever the cut leaves).
All streams are judged by zlib (the tests assert it of the expected bytes here as well)."""
import random
import zlib

from tests import synth
from tests import token_programs as T

SIZES = (0, 1, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289, 16383, 16384, 16385, 20480, 32767, 32768, 32769, 65535, 65536)
LENGTHS = tuple(range(3, 41)) + (255, 256, 257, 258)
DISTANCES = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33)
_BUILT = {}


def _raw(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def _level0_then_6(data):
    """the first half as stored blocks that do not end the stream, the second half as a level-6 stream of its own behind them"""
    h = len(data) // 2
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    return co.compress(data[:h]) + co.flush(zlib.Z_FULL_FLUSH) + _raw(data[h:], 6)


def sizes():
    """[(name, stream, bytes)], built once per process"""
    if "sizes" not in _BUILT:
        text = synth.bench_corpus()[0]
        out = []
        for k, n in enumerate(SIZES):
            o = (k * 7919) % 4096
            d = bytes(text[o:o + n])
            assert len(d) == n
            out.append(("size%d/level6" % n, _raw(d, 6), d))
            out.append(("size%d/stored4000" % n, T.stored_blocks(d, 4000), d))
            out.append(("size%d/stored" % n, T.stored_blocks(d), d))
            out.append(("size%d/level0+6" % n, _level0_then_6(d), d))
        _BUILT["sizes"] = out
    return _BUILT["sizes"]


def _case(rnd, ln, d, k, i):
    return T._lits(rnd, max(d, k)) + [(ln, d)] + T._lits(rnd, 5 if (k + i) & 1 else 0)


def tails():
    """[(name, stream, bytes)], built once per process: per distance one program per placement, every length in it"""
    if "tails" not in _BUILT:
        out = []
        for d in DISTANCES:
            rnd = random.Random(9000 + d)
            near = [t for i, ln in enumerate(LENGTHS) for t in _case(rnd, ln, d, (i + d) % 16, i)]
            far = T._lits(rnd, 6144) + [t for i, ln in enumerate(LENGTHS) for t in _case(rnd, ln, d, (i + 3 * d) % 16, i)]
            split = T._lits(rnd, 6144)
            pos, i = 6144, 0
            while pos < 6144 + 3 * 4096 + 300:
                ln = LENGTHS[(i * 5 + d) % len(LENGTHS)]
                split.append((ln, d))
                split += T._lits(rnd, 1 + i % 3)
                pos += ln + 1 + i % 3
                i += 1
            for what, toks, kind in (("near", near, "fixed"), ("far", far, "dynamic"), ("split", split, "dynamic" if d & 1 else "fixed")):
                prog = [(kind, toks, True, {"shape": "huff", "rle": d % 2 == 0})] if kind == "dynamic" else [(kind, toks, True)]
                out.append(("tails/D%d/%s" % (d, what), T.encode(prog), T.expand(prog)))
        _BUILT["tails"] = out
    return _BUILT["tails"]


def all_entries():
    return sizes() + tails()
