"""tests/bzip2_tokens.py, the structural reader the bzip2 encoder is judged with, held against libbz2's own output
(bz2.compress) and against the writer's programs (bzip2_blocks.verdicts() with status 0): what it reads must decode -- through
bzip2_blocks' ibwt / unrle1 -- to what libbz2 decodes, block CRCs and the combined CRC must be the stored ones, and its
rotation sort must agree with the plain one."""
import bz2

import numpy as np
import pytest

from tests import bzip2_blocks as bb
from tests import bzip2_tokens as bt


def decode(s):
    """the bytes a read() result stands for, with every CRC checked"""
    out, comb = bytearray(), 0
    for b in s["blocks"]:
        chunk = bb.unrle1(bb.ibwt(b["last"], b["orig"]))
        assert chunk is not None and bb.block_crc(chunk) == b["crc"]
        comb = bb.rotl1(comb) ^ b["crc"]
        out += chunk
    assert comb == s["combined"]
    return bytes(out)


def test_compressor_output():
    for name, z, d in bb.payloads():
        s = bt.read(z)
        assert s["level"] == int(name[-1]) and s["in_used"] == len(z) and 0 <= s["pad_bits"] <= 7, name
        assert decode(s) == d, name
        for b in s["blocks"]:
            assert 2 <= b["n_groups"] <= 6 and len(b["tables"]) == b["n_groups"], name
            assert len(b["selectors"]) == (len(b["symbols"]) + 49) // 50, name
            assert b["symbols"][-1] == len(b["used"]) + 1 and b["symbols"] == bb.mtf_symbols(b["last"], b["used"]), name
            for lens in b["tables"]:
                assert 1 <= min(lens) and max(lens) <= 17 and bt.kraft(lens) <= 1 << 32, name
    assert len(bt.read(dict((n, z) for n, z, _ in bb.payloads())["three_blocks_l1"])["blocks"]) == 3
    assert bt.read(bz2.compress(b"", 9))["blocks"] == []


def test_writer_programs():
    seen = 0
    for name, z, st, data, used in bb.verdicts():
        if st != 0:
            continue
        s = bt.read(z)
        assert s["in_used"] == used, name
        if name in ("lengths_oversubscribed",):
            continue
        assert decode(s) == data, name
        seen += 1
    assert seen >= 30
    six = bt.read(dict((v[0], v[1]) for v in bb.verdicts())["six_groups"])["blocks"][0]
    assert six["n_groups"] == 6 and six["selectors"][:7] == [0, 1, 2, 3, 4, 5, 0]
    twenty = bt.read(dict((v[0], v[1]) for v in bb.verdicts())["lengths_20"])["blocks"][0]
    assert set(twenty["tables"][0]) == {20} and bt.kraft(twenty["tables"][0]) < 1 << 32


def test_malformed():
    z = bz2.compress(b"hello hello hello", 9)
    for cut in (0, 3, 10, len(z) - 1):
        with pytest.raises(bt.Malformed):
            bt.read(z[:cut])
    with pytest.raises(bt.Malformed):
        bt.read(b"BZx" + z[3:])


def test_rotation_sort_agrees_with_the_plain_one():
    rs = np.random.RandomState(5)
    for d in (b"a", b"ab", b"banana", b"abab" * 9, b"abc" * 50 + b"ab", rs.bytes(777), bb._text(1500), b"\0" * 300 + b"\1" + b"\0" * 299):
        last, orig = bt.bwt(d)
        want, _ = bb.bwt(d)
        assert last == want
        assert bb.ibwt(last, orig) == d
    assert bt.n_symbols(b"ab") == len(bb.mtf_symbols(bb.bwt(b"ab")[0], [97, 98]))
