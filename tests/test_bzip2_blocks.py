"""CPU tests of the bzip2 stream writer (tests/bzip2_blocks.py) against libbz2 (Python's bz2), both ways: libbz2 decodes
what the writer calls valid to the same bytes and refuses what it calls broken, and the writer's reader half re-reads
bz2.compress output and agrees with libbz2 on every program.  The decoders under test (tests/test_bzip2_emul.py,
tests/test_gpu_bzip2.py) are judged by libbz2 on the same programs."""
import bz2

import pytest

from tests import bzip2_blocks as bb

T = bb._text(700)


def test_families_present():
    names = {n for n, _, _ in bb.PROGRAMS()}
    for want in ("plain", "level_1", "orig_ptr_nblock", "randomised", "map_superset", "n_groups_7", "n_selectors_0",
                 "selector_value_nGroups", "lengths_flat_incomplete", "lengths_oversubscribed", "lengths_20", "length_0", "length_21",
                 "run_weights_22", "symbols_over_capacity", "no_end_of_block", "block_crc", "combined_crc", "block_magic",
                 "end_magic", "count_252", "count_255", "four_at_end_no_count", "four_split_across_blocks", "trailing"):
        assert want in names
    assert sum(n.startswith("cut_") for n in names) >= 20


def test_libbz2_agrees_with_the_writers_claims():
    """every program the writer calls valid / broken / cut short gets that verdict from libbz2 (randomised blocks apart:
    libbz2 decodes them, the decoders here refuse them)"""
    for name, stream, want in bb.PROGRAMS():
        st, out, used = bb.judge(stream)
        if want == bb.UNSUPPORTED:
            assert st in (bb.OK, bb.DATA_ERROR), name
        elif want is not None:
            assert st == want, (name, st, want)


def test_valid_programs_decode_to_their_bytes():
    assert bz2.decompress(bb.write_stream([bb.block(T)])) == T
    assert bz2.decompress(bb.write_stream([bb.block(T[:300]), bb.block(T[300:])], level=1)) == T
    assert bz2.decompress(bb.write_stream([])) == b""
    assert bz2.decompress(bb.write_stream([bb.block(b"q" * 1000 + b"r" * 3 + b"s" * 4)])) == b"q" * 1000 + b"r" * 3 + b"s" * 4
    assert bz2.decompress(bb.write_stream([bb.block(pre=b"x" + b"q" * 4 + b"\xff" + b"y")])) == b"x" + b"q" * 259 + b"y"
    assert bz2.decompress(bb.write_stream([bb.block(pre=b"xyqq"), bb.block(pre=b"qq\x05z")])) == b"xyqqqq\x05z"
    d = bz2.BZ2Decompressor()
    assert d.decompress(bb.write_stream([bb.block(T)], trailing=b"behind")) == T and d.unused_data == b"behind"


def test_reader_half_agrees_with_libbz2_on_every_program():
    for name, stream, want in bb.PROGRAMS():
        st, out, used = bb.judge(stream)
        got = bb.read_stream(stream)
        if want == bb.UNSUPPORTED:
            assert got[0] == bb.UNSUPPORTED, name
            continue
        assert got[0] == st, (name, got[0], st)
        if st == 0:
            assert got[1] == out and got[2] == used, name


@pytest.mark.parametrize("level", [1, 9])
def test_reader_half_rereads_the_compressor(level):
    for name, z, d in bb.payloads():
        if len(d) <= 20000:
            assert bb.read_stream(z) == (0, d, len(z)), name
    z = bz2.compress(T * 3, level)
    assert bb.read_stream(z + b"tail") == (0, T * 3, len(z))
    assert bb.read_stream(z[:-1])[0] == bb.BUF_ERROR
    assert bb.read_stream(z[:-5] + bytes([z[-5] ^ 1]) + z[-4:])[0] == bb.DATA_ERROR


def test_rle1_and_bwt_round_trip():
    for d in (b"", b"a", b"aaaa", b"aaaaa", b"a" * 255, b"a" * 256, b"a" * 600, T, b"abab" * 10):
        pre = bb.rle1(d)
        assert bb.unrle1(pre) == d
        last, orig = bb.bwt(pre)
        if pre:
            assert bb.ibwt(last, orig) == pre
    assert bb.unrle1(b"xyqqqq") is None
    assert bb.block_crc(b"123456789") == 0xFC891918
