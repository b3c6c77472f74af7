"""Cases for the refill of K1's two walks (minizip-ng_amd/csrc/inflate_walk.inc: the edge groups in a branch of their own, one
check per trip of four steps): what the refill decides depends on where the input ENDS relative to the aligned groups of four
dwords the ring is topped up in, and on how fast a lane eats its ring.  Shared by tests/test_walk_refill_emul.py (the host
emulation at the product's caps and at low ones, and the sanitised stand-alone program) and tests/test_gpu_walk_refill.py (the
device).  zlib's inflate is the judge of every case.

    streams()   level-6 streams of 300 B .. 8 KiB of output whose lengths take every residue mod 16, plus one of 64 KiB (a
                window with all 64 spans)
    cuts()      every stream cut at every byte of its last 48
    wide()      dynamic blocks whose literal, length and distance codes are all 15 bits long, the matches with 5 and 13 extra
                bits: a step (leading literal + match) is 63 bits, the most a step can be.  "sustained": nothing but such
                steps, spans of more than 1 024 bits (two rings) and every span boundary inside them; "drift": runs of them
                between runs of 1-bit literals, so that the lanes of a wave stand at different distances from their refills
"""
import random
import zlib

from tests import synth
from tests import token_programs as T

CUT_BYTES = 48
_BUILT = {}


def verdict(z, cap):
    """zlib's: (status, consumed input, bytes).  0 = the stream ends inside z; -3 = zlib refuses it; -5 = z ends first"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z, cap + 1)
    except zlib.error:
        return -3, 0, b""
    if not d.eof:
        return -5, 0, out
    assert len(out) <= cap
    return 0, len(z) - len(d.unused_data), out


def streams():
    """[(name, stream, bytes)]: one stream per residue of len(stream) mod 16, output sizes spread over 300 B .. 8 KiB; and 64 KiB"""
    if "streams" in _BUILT:
        return _BUILT["streams"]
    c = synth.corpus()
    rnd = random.Random(916)
    sizes = [300 + (8192 - 300) * k // 15 for k in range(16)]
    out = []
    for r in range(16):
        for _ in range(400):                       # (more candidates than needed: the first whose length has residue r)
            n = sizes[r] + rnd.randrange(-40, 41) if r not in (0, 15) else sizes[r]
            o = rnd.randrange(len(c) - n)
            z = synth.deflate_raw(c[o:o + n])
            if len(z) % 16 == r:
                out.append(("text/%dB/len%%16=%d" % (n, r), z, c[o:o + n]))
                break
        else:
            raise AssertionError("no stream with length residue %d" % r)
    o = rnd.randrange(len(c) - 65536)
    out.append(("text/64KiB", synth.deflate_raw(c[o:o + 65536]), c[o:o + 65536]))
    assert {len(z) % 16 for _, z, _ in out[:16]} == set(range(16))
    assert min(len(d) for _, _, d in out) == 300 and sorted(len(d) for _, _, d in out)[-2] == 8192
    _BUILT["streams"] = out
    return out


def cuts():
    """[(name, stream, room for the whole stream's bytes)]: every stream of streams() without its last 1 .. CUT_BYTES bytes"""
    if "cuts" not in _BUILT:
        _BUILT["cuts"] = [("%s/cut-%d" % (name, k), z[:len(z) - k], len(d)) for name, z, d in streams() for k in range(1, CUT_BYTES + 1)]
    return _BUILT["cuts"]


_WIDE_LITS = (0x41, 0x5A, 0x00, 0xFF)
_SHORT_LIT = 0x20


def _history_block(rnd):
    """32 KiB + 1 of output from a few hundred bits: what the 13-extra-bit distances reach back into"""
    return ("fixed", [rnd.randrange(256)] + [(258, 1)] * 127, False)


def _wide_step(rnd):
    ln = rnd.randrange(227, 259)                    # symbol 284: five extra bits (258 as 284 + 31, not as symbol 285)
    return [rnd.choice(_WIDE_LITS), (258, 16385 + rnd.randrange(16384), True) if ln == 258 else (ln, 16385 + rnd.randrange(16384))]


def _wide_opts(short=False):
    lens = {s: 15 for s in _WIDE_LITS + (284, 256)}
    if short:
        lens[_SHORT_LIT] = 1
    dlens = {s: s + 1 for s in range(14)}           # a complete distance code: 1 .. 14 bits for symbols nobody uses, 15 for the two with 13 extra bits
    dlens[28] = dlens[29] = 15
    return {"lens": lens, "dlens": dlens}


def wide():
    """[(name, stream, bytes)] of the two wide-step programs"""
    if "wide" in _BUILT:
        return _BUILT["wide"]
    rnd = random.Random(917)
    toks = []
    for _ in range(1700):                           # 107 100 bits of 63-bit steps: 64 spans of ~1 680 bits
        toks += _wide_step(rnd)
    sustained = [_history_block(rnd), ("dynamic", toks, True, _wide_opts())]
    toks, bits = [], 0
    while bits < 110000:                            # runs of wide steps between runs of one-bit literals
        if rnd.random() < 0.5:
            for _ in range(rnd.choice((1, 1, 2, 3, 4, 5, 8, 17, 40))):
                toks += _wide_step(rnd)
                bits += 63
        else:
            n = rnd.choice((1, 2, 3, 4, 7, 31, 32, 33, 64, 200))
            toks += [_SHORT_LIT] * n
            bits += n
    drift = [_history_block(rnd), ("dynamic", toks, True, _wide_opts(short=True))]
    out = []
    for name, prog in (("wide/sustained", sustained), ("wide/drift", drift)):
        lit, dist = T.block_lengths(prog[1][1], prog[1][3])
        assert all(lit[s] == 15 for s in _WIDE_LITS + (284, 256)) and dist[28] == dist[29] == 15, name
        z, data = T.encode(prog), T.expand(prog)
        assert verdict(z, len(data)) == (0, len(z), data), name
        out.append((name, z, data))
    _BUILT["wide"] = out
    return out


def everything():
    """[(name, stream, expected bytes or None, zlib's status, zlib's consumed input, out_cap)], computed once"""
    if "all" not in _BUILT:
        out = []
        for name, z, data in streams() + wide() + cuts():
            cap = data if isinstance(data, int) else len(data)
            st, used, got = verdict(z, cap)
            if not isinstance(data, int):
                assert (st, used, got) == (0, len(z), data), name
            out.append((name, z, got if st == 0 else None, st, used, cap))
        _BUILT["all"] = out
    return _BUILT["all"]
