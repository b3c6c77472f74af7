"""Cases for two parts of K1: the chase of pass 2 (minizip-ng_amd/csrc/inflate_walk.inc: a chase takes its next target in front
of a trip of four steps, not inside a step) and the set-up of the near batches (inflate_commit.inc: the rank searches on byte
offsets, the short-period prologue from a packed constant).  Shared by tests/test_chase_lean_emul.py (the host emulation at the
product's caps and at low ones, and the sanitised stand-alone program) and tests/test_gpu_chase_lean.py (the device).  Every case
is a stream zlib accepts; zlib's bytes are the expected ones (the tests assert it).

    retarget()   where a chase runs through whole spans: level-1/6/9 text of 300 .. 2 000 bytes (spans at the 128-bit floor,
                 two to six steps each); 63-bit steps under 128-bit spans (a chase is in the next span but one after two steps,
                 and out of targets in the middle of a trip); stored and fixed blocks between dynamic ones and blocks of 5 .. 40
                 tokens (an end of block inside almost every chase, target walks that ended with it); random literals under a
                 flat 8-bit code (a lane that starts off the byte phase never meets anybody: every chase runs into
                 MZ_REC_CAP2) and under 1- and 2-bit codes (own walks run into MZ_REC_CAP1: targets that ended with the cap);
                 fixed blocks of random bytes (a walk from a wrong phase meets the codes zlib refuses: targets that ended
                 with an invalid code)
    near()       every distance 1 .. 7 (and 8, 9, 16 next to them) with every match length 3 .. 34 -- near pieces of 1 .. 32
                 bytes, shorter than the prologue D8 - D and longer -- behind 0 .. 16 fresh literals, so that with the output
                 misalignments of the tests pieces start at staging index 0, 15, 16; runs of 258-byte matches at distance
                 1 .. 7 over more than two chunks (pieces up to the last staging byte, batches of 64 pieces that each wait for the
                 one before: dependency depth 64; a last batch with fewer than 64, so the fillers take part in the search);
                 and the tails of tests/commit_chain_cases.py
"""
import random
import zlib

from tests import commit_chain_cases as K
from tests import token_programs as T

_BUILT = {}
TEXT_SIZES = (300, 317, 411, 500, 640, 777, 901, 1000, 1234, 1500, 1777, 2000)


def _raw(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def _text(rnd, n):
    words = [bytes(rnd.choice(b"etaoinshrdlucmfwyp") for _ in range(rnd.randint(2, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + rnd.choice((b" ", b" ", b", ", b".\n"))
    return bytes(out[:n])


def _prog(name, prog):
    return name, T.encode(prog), T.expand(prog)


def retarget():
    """[(name, stream, bytes)], built once per process"""
    if "retarget" in _BUILT:
        return _BUILT["retarget"]
    out = []
    rnd = random.Random(1001)
    for n in TEXT_SIZES:
        d = _text(rnd, n)
        for lvl in (1, 6, 9):
            out.append(("retarget/text%d/level%d" % (n, lvl), _raw(d, lvl), d))
    # long steps under short spans: 300 .. 2 000 bytes of output in steps of a literal and a long far match
    from tests import walk_refill_cases as W
    for k, steps in enumerate((3, 6, 12, 24, 60)):
        r = random.Random(1100 + k)
        body = []
        for i in range(steps):
            body += W._wide_step(r) + [W._SHORT_LIT] * ((i * 3 + k) % 5)
        out.append(_prog("retarget/wide%d" % steps, [W._history_block(r), ("dynamic", body, True, W._wide_opts(short=True))]))
    # stored and fixed blocks in the middle; short blocks
    for k in range(6):
        r = random.Random(1200 + k)
        a, b, c = T._lits(r, 150 + 40 * k), T._lits(r, 90 + 17 * k), T._lits(r, 200)
        m = [(3 + (7 * i + k) % 30, 1 + (11 * i + k) % 120) for i in range(25)]
        prog = [("dynamic", a + m[:8], False, {"shape": "huff"}), ("stored", bytes(T._lits(r, 33 + k)), False), ("dynamic", b + m[8:16], False, {"shape": "deep"}),
                ("fixed", c + m[16:], False), ("dynamic", T._lits(r, 120) + m[:5], True, {"shape": "flat"})]
        out.append(_prog("retarget/mixed-blocks%d" % k, prog))
    for k in range(4):
        r = random.Random(1300 + k)
        toks = []
        for i in range(700):
            toks += T._lits(r, 1 + i % 3)
            if i > 120 and i % 2:
                toks.append((3 + (i * 5) % 20, 1 + (i * 13) % 200))
        prog = T.cut_into_blocks(toks, r, lo=5, hi=40, stored_every=7 if k & 1 else 0, empty_every=11 if k & 2 else 0)
        out.append(_prog("retarget/short-blocks%d" % k, prog))
    # no meeting point: fixed-length codes, lanes off the phase chase until the record cap; 1- and 2-bit codes: own walks capped
    r = random.Random(1400)
    out.append(_prog("retarget/flat8-cap2", [("dynamic", T._lits(r, 30000), True, {"shape": "flat"})]))
    out.append(_prog("retarget/flat8-small", [("dynamic", T._lits(r, 1500), True, {"shape": "flat"})]))
    two = [r.choice((65, 65, 65, 66)) for _ in range(60000)]
    out.append(_prog("retarget/short-codes-cap1", [("dynamic", two, True, {"shape": "huff"})]))
    # fixed blocks of random bytes: invalid codes off the phase
    for k, n in enumerate((400, 1900, 9000)):
        r = random.Random(1500 + k)
        toks = []
        for i in range(n // 4):
            toks += T._lits(r, 3)
            if i > 10 and i % 3 == 0:
                toks.append((3 + i % 9, 1 + (i * 7) % 30))
        out.append(_prog("retarget/fixed-random%d" % n, [("fixed", toks, True)]))
    _BUILT["retarget"] = out
    return out


NEAR_DISTANCES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16)
NEAR_LENGTHS = tuple(range(3, 35))


def near():
    """[(name, stream, bytes)], built once per process"""
    if "near" in _BUILT:
        return _BUILT["near"]
    out = []
    for d in NEAR_DISTANCES:
        for k in (0, 1, 15, 16):                       # fresh literals in front: where the first piece starts in the staging area
            r = random.Random(2000 + 17 * d + k)
            toks = []
            for i, ln in enumerate(NEAR_LENGTHS):
                toks += T._lits(r, max(d, k if i == 0 else (i * 5 + d) % 17)) + [(ln, d)]
            kind = "fixed" if (d + k) & 1 else "dynamic"
            out.append(_prog("near/D%d/lits%d" % (d, k), [(kind, toks, True, {"shape": "huff"})] if kind == "dynamic" else [(kind, toks, True)]))
    for d in range(1, 8):                              # long runs: chunks full of pieces that each read the one before
        r = random.Random(2100 + d)
        toks = T._lits(r, d + (d * 3) % 16) + [(258, d)] * (34 + d) + T._lits(r, 3) + [(3 + d, d)]
        out.append(_prog("near/D%d/run" % d, [("dynamic", toks, True, {"shape": "flat"})]))
    out += [e for e in K.tails() if "/near" in e[0] or "/split" in e[0]]
    _BUILT["near"] = out
    return out


def everything():
    """[(name, stream, bytes, out_cap)]; the capacity is the size, or some bytes more"""
    if "all" not in _BUILT:
        _BUILT["all"] = [(n, z, d, len(d) + (0 if i % 2 == 0 else 1 + (i * 7) % 64)) for i, (n, z, d) in enumerate(retarget() + near())]
    return _BUILT["all"]
