"""CPU tests of the token walker itself (tests/deflate_tokens.py): it reads what zlib writes, it measures the property
include/mzhip.h words its window promise in (zlib's own MAX_DIST), and it refuses what RFC 1951 forbids -- never less than
zlib refuses."""
import zlib

import pytest

from tests import synth
from tests.deflate_tokens import DeflateError, stored_cost_bits, walk
from tests.test_oracle import INCOMPLETE_DISTANCE_SET
from tests.token_programs import _Bits, _canonical, dynamic_block  # noqa: F401  (the writers live in the token-program helper)


def _zlib(z):
    """-> the bytes zlib's raw inflate makes of z, None if it refuses z or z ends before its final block"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(z)
    except zlib.error:
        return None
    return out if d.eof else None


def _refused(z, **kw):
    with pytest.raises(DeflateError) as e:
        walk(z, **kw)
    return str(e.value)


def test_walker_reads_what_zlib_writes():
    cases = synth.edge_payloads() + synth.long_code_payloads(20000)
    c = synth.corpus()
    cases += [("stored/%d" % blk, c[:n], synth.stored_blocks(c[:n], block=blk)) for n, blk in ((0, 65535), (1, 65535), (3000, 1000), (65535, 65535),
                                                                                              (65536, 65535), (140000, 65535))]
    kinds = {}
    for name, data, z in cases:
        w = walk(z, data=True)
        assert w.data == data and w.out_len == len(data), name
        assert (w.bits + 7) // 8 == len(z) and w.blocks[-1].end_bit == w.bits, name
        assert [b.bfinal for b in w.blocks] == [0] * (len(w.blocks) - 1) + [1], name
        pos = bit = 0
        for b in w.blocks:                                   # blocks follow each other without a gap, in bits and in bytes
            assert (b.first_bit, b.out_start) == (bit, pos) and b.end_bit > b.first_bit and b.out_end >= b.out_start, name
            bit, pos = b.end_bit, b.out_end
        assert pos == len(data), name
        m = w.matches
        if len(m):
            assert m[:, 1].min() >= 3 and m[:, 1].max() <= 258 and m[:, 2].min() >= 1 and (m[:, 2] <= m[:, 0]).all(), name
            assert (m[1:, 0] >= m[:-1, 0] + m[:-1, 1]).all(), name
        assert walk(z).matches.tolist() == m.tolist() and walk(z).data is None, name     # the same tokens without the bytes
        kinds[name] = {b.btype for b in w.blocks}
    assert kinds["text_fixed"] == {1} and kinds["stored_only"] == {0} and kinds["stored_empty"] == {0}
    assert all(k == {0} for n, k in kinds.items() if n.startswith("stored/"))
    assert kinds["random_incompressible"] == {0} and kinds["text_64k_l6"] == {2} and kinds["sync_flushed"] == {0, 2}
    assert all(k == {2} for n, k in kinds.items() if n.startswith("geom"))
    w = walk(dict(synth.hand_made())["dist_32768"])           # (zlib never writes the largest distance: a stream made by hand)
    assert w.matches.tolist() == [[32768, 258, 32768], [32768 + 258, 3, 32768], [32768 + 262, 100, 32768]]
    # stored blocks of the largest size cost what stored_cost_bits says, less the padding an aligned block does not need
    w = walk(synth.stored_blocks(c[:140000]))
    assert [b.end_bit - b.first_bit for b in w.blocks] == [stored_cost_bits(b.out_end - b.out_start) - 7 for b in w.blocks]


@pytest.mark.parametrize("wbits", range(9, 16))
def test_walker_measures_zlibs_window(wbits):
    """zlib's own property, in the words of include/mzhip.h: a raw stream made with windowBits w has no distance beyond
    2^w - 262 (MAX_DIST) -- on the inputs that offer matches at, just below and just above it -- and comes close to it."""
    bound = (1 << wbits) - 262
    far = 0
    for level in (1, 6, 9):
        for name, d, period in synth.echo_cases(wbits):
            co = zlib.compressobj(level, zlib.DEFLATED, -wbits)
            z = co.compress(d) + co.flush()
            w = walk(z, data=True)
            assert w.data == d, (level, name)
            if len(w.matches):
                assert w.matches[:, 2].max() <= bound, (level, name, int(w.matches[:, 2].max()))
                far = max(far, int(w.matches[:, 2].max()))
    assert far > bound - 16, (far, bound)


def _lens(pairs, n):
    out = [0] * n
    for s, l in pairs.items():
        out[s] = l
    return out


def test_walker_refuses_what_rfc1951_forbids():
    c = synth.corpus()
    z = synth.deflate_raw(c[:3000])
    stored = synth.stored_blocks(c[:3000], block=1000)
    two = _lens({97: 2, 98: 2, 257: 2, 256: 2}, 258)         # a, b, length 3, end of block: a complete set
    open_fixed = synth.fixed_stream(list(c[:50]))
    bad = {       # name: (stream, what the message must say)
        "block type 3": (bytes([z[0] | 0x06]) + z[1:], "block type 3"),
        "stored, NLEN": (stored[:1005] + bytes([stored[1005], stored[1006], stored[1007] ^ 1]) + stored[1008:], "NLEN"),
        "length symbol 286": (synth.fixed_stream(list(c[:300]) + [286] + list(c[300:400])), "286 or 287"),
        "length symbol 287": (synth.fixed_stream(list(c[:30]) + [287]), "286 or 287"),
        "distance symbol 30": (_fixed_with_distance_symbol(30), "30 or 31"),
        "distance symbol 31": (_fixed_with_distance_symbol(31), "30 or 31"),
        "distance at position 0": (synth.fixed_stream([(258, 1), 65, 66]), "in front of the first byte"),
        "distance 101 at position 100": (synth.fixed_stream(list(c[:100]) + [(3, 101), 67]), "in front of the first byte"),
        "cut in half": (z[:len(z) // 2], "input ends"), "one byte short": (z[:-1], "input ends"), "no input": (b"", "input ends"),
        "cut in a stored block": (stored[:1500], "input ends"),
        "no final block": (bytes([open_fixed[0] & 0xFE]) + open_fixed[1:], "input ends"),
        "over-subscribed literal set": (dynamic_block(_lens({97: 1, 98: 1, 256: 1}, 257), [1], [97, 256]), "literal/length code set is over-subscribed"),
        "over-subscribed distance set": (dynamic_block(two, [1, 1, 1], [97, 256]), "distance code set is over-subscribed"),
        "incomplete literal set": (dynamic_block(_lens({97: 1, 256: 2}, 257), [1], [97, 256]), "literal/length code set is incomplete"),
        "incomplete distance set": (dynamic_block(two, [2, 2], [97, 256]), "distance code set is incomplete"),
        "one distance code of two bits": (dynamic_block(two, [2], [97, 256]), "distance code set is incomplete"),
        "no code for end-of-block": (dynamic_block(_lens({97: 1, 98: 1}, 257), [1], [97, 98]), "end-of-block"),
        "no literal code at all": (dynamic_block([0] * 257, [1], []), "end-of-block"),
        "287 literal/length codes": (dynamic_block(_lens({97: 1, 256: 1}, 287), [1], [97, 256], hlit=287), "more than 286"),
        "the other code of a one-code distance set": (dynamic_block(two, [1], [97, 98, 97, 257, ("d", 1)]), "distance code that no symbol has"),
        "a match in a block without distance codes": (dynamic_block(two, [0], [97, 98, 97, 257, ("d", 0)]), "distance code that no symbol has"),
    }
    for name, (s, says) in bad.items():
        assert says in _refused(s), (name, _refused(s))
        assert _zlib(s) is None, name                     # (nothing here is stricter than zlib)
    for s in INCOMPLETE_DISTANCE_SET:                         # the device fuzz's find: a match takes the unused code of a one-code set
        assert "distance code that no symbol has" in _refused(s) and _zlib(s) is None
    # ... and what zlib's exception allows is read: one distance code of one bit, or none at all in a block without matches
    ok = dynamic_block(two, [1], [97, 98, 97, 257, ("d", 0), 256])
    assert walk(ok, data=True).data == _zlib(ok) == b"abaaaa"
    ok = dynamic_block(two, [0], [97, 98, 256])
    assert walk(ok, data=True).data == _zlib(ok) == b"ab"
    # history: a distance may reach that far in front of the stream and no further
    far = synth.fixed_stream(list(c[:100]) + [(3, 101), 67])
    w = walk(far, history=1, data=True, prefix=b"Q")
    assert w.data == c[:100] + b"Q" + c[:2] + b"C" and w.matches.tolist() == [[100, 3, 101]]
    assert "in front of the first byte" in _refused(synth.fixed_stream(list(c[:100]) + [(3, 102), 67]), history=1)
    # a piece that is not final: the input may end between blocks on a byte boundary, nowhere else
    piece = bytes([far[0] & 0xFE]) + far[1:]
    assert "input ends" in _refused(piece, history=1) and "input ends" in _refused(piece, history=1, open_end=True)
    spare = -walk(far, history=1).bits % 8            # zero bits behind the block in its last byte: room for the next header?
    piece += (b"" if spare >= 3 else b"\x00") + b"\x00\x00\xff\xff"
    assert "input ends" in _refused(piece, history=1)
    w = walk(piece, history=1, open_end=True)
    assert [(b.btype, b.bfinal, b.out_end - b.out_start) for b in w.blocks] == [(1, 0, 104), (0, 0, 0)] and w.bits == 8 * len(piece)


def _fixed_with_distance_symbol(sym):
    """a final fixed block: 'A', then a match of length 3 whose distance symbol is `sym` (30 and 31 have codes and no meaning)"""
    b = _Bits()
    b.put(1, 1)
    b.put(1, 2)
    b.code(0x30 + 65, 8)
    b.code(257 - 256, 7)
    b.code(sym, 5)
    b.put(0, 13)
    b.code(0, 7)
    return b.bytes()


def test_walker_agrees_with_zlib_on_the_suites_streams():
    """The hand-made streams (fixed blocks with chosen tokens, distance 32768 among them) and the corruptions the decoder
    tests use: whatever zlib refuses, or does not see the end of, the walker refuses; what zlib reads, the walker reads alike."""
    for name, z in synth.hand_made():
        assert walk(z, data=True).data == _zlib(z) is not None, name
    n_bad = n_ok = 0
    for name, data, z in synth.edge_payloads():
        if len(z) < 16:
            continue
        for cname, bad in synth.corruptions(z):
            want = _zlib(bad)
            try:
                got = walk(bad, data=True).data
            except DeflateError:
                got = None
            if want is None:
                assert got is None, (name, cname)
                n_bad += 1
            else:                      # (a flipped bit often leaves a valid stream of other bytes)
                assert got == want, (name, cname)
                n_ok += 1
    assert n_bad > 50 and n_ok > 50, (n_bad, n_ok)
