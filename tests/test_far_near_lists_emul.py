"""CPU tests of the far and near lists of K1's commit (inflate_emit.inc classes every piece of a back-reference as far only, near
only or split and writes two lists; inflate_commit.inc copies the far list from the output buffer, then the near list inside the
staging area) on the 64-lane host emulation of the shipped sources, tests/emul/far_near_main.cpp built with -DMZ_STATS.  The
entries are tests/far_near_cases.py's; zlib judges status, bytes, consumed input and CRC-32, the kernel's own counters say
which entries a decode made, and every decode runs between red zones around its output, its record scratch and its LDS.

What the counters can and cannot say: they are sums over the chunks of one decode.  Every piece makes one entry, a split one
two, so far entries + near entries == pieces + split pieces, exactly, for every case (every match of every case stands more
than 300 literals in front of the stream's end, so none is left to the step loop, which makes no entries); near entries ==
near-only pieces + split pieces is held exactly wherever model() or the construction gives the classes.  Where the far entries
of a case lie in one chunk, far batches == ceil(far entries / 64) exactly; over several chunks the sum of the chunks' ceilings
is only bounded by the sums: ceil(F / 64) <= batches <= ceil(F / 64) + chunks - 1.

Counter 21 (split pieces) is counted where the emit writes the entries, so it also counts the split pieces of a round that a
distance in front of the entry then refuses (test_distance_in_front_of_the_entry).

The last test compiles the same file as a program of its own with -fsanitize=address,undefined and runs it as a child process."""
import os
import struct
import subprocess
import zlib

import pytest

from tests import far_near_cases as FN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ceil64(n):
    return (n + 63) // 64


def _decode_and_judge(c, omis):
    """one decode of an accepted case: zlib's four words and bytes, red zones intact -> the counters"""
    words, out, s, intact = FN.decode(c["z"], c["cap"], omis=omis)
    assert intact, (c["name"], omis)
    assert words == (0, len(c["data"]), len(c["z"]), zlib.crc32(c["data"])), (c["name"], omis, words)
    if out != c["data"]:
        bad = next(k for k in range(len(out)) if out[k] != c["data"][k])
        raise AssertionError("%s (omis %d): byte %d of %d is %d, zlib says %d" % (c["name"], omis, bad, len(out), out[bad], c["data"][bad]))
    far, near = s[FN.ENTRIES] - s[FN.NEAR], s[FN.NEAR]
    # the counters among themselves: near pieces = near only + split, so at least the split ones; a batch per 64 entries and chunk
    assert near >= s[FN.SPLIT] and far >= s[FN.SPLIT], (c["name"], far, near, s[FN.SPLIT])
    assert _ceil64(far) <= s[FN.FAR_BATCHES] <= _ceil64(far) + max(s[FN.CHUNKS], 1) - 1, (c["name"], far, s[FN.FAR_BATCHES], s[FN.CHUNKS])
    assert _ceil64(near) <= s[FN.NEAR_BATCHES] <= _ceil64(near) + max(s[FN.CHUNKS], 1) - 1, (c["name"], near, s[FN.NEAR_BATCHES])
    assert far + near == c["pieces"] + s[FN.SPLIT], (c["name"], far, near, c["pieces"], s[FN.SPLIT])
    assert s[FN.BYTES] <= len(c["data"])
    return s, far, near


def test_cases_are_zlibs():
    names = set()
    for c in FN.accepted():
        d = zlib.decompressobj(-15)
        assert d.decompress(c["z"]) == c["data"] and d.eof and d.unused_data == b"", c["name"]
        assert len(c["data"]) <= 65536
        names.add(c["name"])
    assert len(names) == len(FN.accepted())
    for c in FN.refused():
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(c["z"])


def test_model_is_the_definition():
    """model() against the three classes spelled out for one piece, and a match of 258 bytes piece by piece"""
    assert FN.model(20, 0) == (0, 1, 0) and FN.model(20, 20) == (1, 0, 0) and FN.model(20, 1) == FN.model(20, 19) == (1, 1, 1)
    assert FN.model(258, 64) == (2, 7, 0) and FN.model(258, 65) == FN.model(258, 95) == (3, 7, 1) and FN.model(258, 96) == (3, 6, 0)
    assert FN.model(258, 257) == (9, 1, 1) and FN.model(258, 258) == (9, 0, 0)


def test_class_edges():
    """dist == dw + len is far only, one less a split with one near byte, dist == dw near only, one more a split with one far
    byte -- for a piece of 20 bytes and for the third piece of a match of 258 -- by the entries the decode made.  The match is
    the stream's only one, so its entries are the decode's, all in one chunk."""
    for k, c in enumerate(FN.edges()):
        for omis in (0, (5 * k + 1) % 16):
            s, far, near = _decode_and_judge(c, omis)
            assert (far, near, s[FN.SPLIT]) == (c["far"], c["near"], c["split"]), (c["name"], omis, far, near, s[FN.SPLIT])
            assert s[FN.FAR_BATCHES] == _ceil64(far) and s[FN.NEAR_BATCHES] == _ceil64(near), c["name"]


def test_chunk_of_split_pieces():
    """Every piece of the train in one chunk split, and more of them than the pool holds at two entries a piece:
      - every match of the stream has a far part (far entries == all pieces), and the near entries are exactly the split pieces:
        counter 21 == the train's pieces of that chunk, each of which left one near entry;
      - the cut shrank: the near-only twin, same bit layout, one entry a piece, holds MORE of the train in the same chunk (its
        near entries; behind the chunk its pieces are far only);
      - the number is what the fit rule allows: lead + 3 S staging bytes (lead = the chunk's bytes in front of the train, the
        LONG matches among them), 4 (9 LONG + 2 S) list bytes and 48 fit a pool of at most 5 104 + 4 x 404 bytes (every
        second-level table entry unused), and one lane more -- eight matches -- does not fit with 15 bytes of misalignment
        in a pool of at least 5 104;
      - the far-only twin makes no near entry at all."""
    cases = FN.all_split()
    assert [c["name"].split("/")[1:] for c in cases] == [[k, v] for k in ("fixed", "dynamic") for v in ("split", "near", "far")]
    for split, near_twin, far_twin in (cases[:3], cases[3:]):
        for omis in (0, 3):
            s, far, near = _decode_and_judge(split, omis)
            S = s[FN.SPLIT]
            assert far == split["pieces"] and near == S and S >= 128, (split["name"], far, near, S)
            lead = split["lead"]
            assert omis + lead + 3 * S + 4 * (9 * FN.LONG + 2 * S) + 48 <= 5104 + 4 * 404, (split["name"], S, lead)
            assert 15 + lead + 3 * (S + 8) + 4 * (9 * FN.LONG + 2 * (S + 8)) + 48 > 5104, (split["name"], S, lead)
            t, tfar, tnear = _decode_and_judge(near_twin, omis)
            assert t[FN.SPLIT] == 0 and tfar + tnear == near_twin["pieces"] and tnear > S, (near_twin["name"], tnear, S)
            t, tfar, tnear = _decode_and_judge(far_twin, omis)
            assert (tfar, tnear, t[FN.SPLIT]) == (far_twin["pieces"], 0, 0), far_twin["name"]


def test_chunks_of_one_kind():
    no_far, no_near = FN.one_kind()
    s, far, near = _decode_and_judge(no_far, 7)
    assert (far, near, s[FN.SPLIT], s[FN.CHUNKS], s[FN.FAR_BATCHES]) == (0, no_far["near"], 0, 1, 0)
    assert s[FN.NEAR_BATCHES] == _ceil64(near)
    s, far, near = _decode_and_judge(no_near, 7)
    assert (far, near, s[FN.SPLIT], s[FN.NEAR_BATCHES]) == (no_near["far"], 0, 0, 0), (far, no_near["far"])


def test_short_period_behind_far_bytes():
    """distance 1 .. 7 across chunk starts: the far bytes are there before the near part's prologue repeats them (zlib's bytes),
    and every entry has split pieces"""
    for c in FN.short():
        for omis in (0, 9):
            s, far, near = _decode_and_judge(c, omis)
            assert s[FN.SPLIT] >= 2 and far >= s[FN.SPLIT], (c["name"], s[FN.SPLIT], far)


def test_distance_in_front_of_the_entry():
    """behind a split piece of the same chunk: the answer of the commit before the two lists, the bytes in front of the token,
    and nothing behind them"""
    (c,) = FN.refused()
    for omis in (0, 13):
        words, out, s, intact = FN.decode(c["z"], c["cap"], omis=omis)
        assert intact and words == FN.REFUSED_PARENT, (omis, words)
        assert out[:words[1]] == c["data"] and words[3] == zlib.crc32(c["data"])
        assert out[words[1]:words[1] + 4] == b"\xA5" * 4          # (the refused match's own bytes; the step loop, which has the verdict,
        #                                                            writes the literals of its step behind them, inside the capacity)
        assert s[FN.SPLIT] >= 1                                   # (the split piece was classed before the round was refused)


def test_sanitised_program(tmp_path):
    """tests/emul/far_near_main.cpp under AddressSanitizer and UBSan, a process of its own: every case at four output
    misalignments from heap blocks that end with the input's last aligned dword and the output's capacity"""
    exe = str(tmp_path / "far_near_main")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul", "far_near_main.cpp"), "-o", exe], check=True)
    cases = FN.accepted() + FN.refused()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<II", len(c["z"]), c["cap"]) + c["z"])
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(lines) == 4 * len(cases)
    for k, _, st, ol, iu, crc in lines:
        c = cases[k]
        want = (0, len(c["data"]), len(c["z"]), zlib.crc32(c["data"])) if k < len(FN.accepted()) else FN.REFUSED_PARENT
        assert (st, ol, iu, crc) == want, (c["name"], st, ol, iu, crc)
