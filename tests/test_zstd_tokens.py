"""The structural reader tests/zstd_tokens.py held against streams it did not write: libzstd's committed ones
(tests/golden/zstd_streams.json) and every valid frame program of tests/zstd_frames.py.  Replaying the sequences it reads
gives the bytes expand() gives; the fields it reports are the ones the programs were written with.  Needs no libzstd."""
import base64
import json

from tests import zstd_frames as zf
from tests import zstd_tokens as zt


def test_committed_streams_replay_to_their_inputs():
    g = zf.golden_inputs()
    with open(zf.GOLDEN) as f:
        streams = json.load(f)
    seen = dict(modes=set(), lit=set(), trees=set(), types=set())
    for name, b64 in streams.items():
        z = base64.b64decode(b64)
        frames = zt.read(z)
        assert sum(f["size"] for f in frames) == len(z), name
        assert zt.replay(frames) == g[name][0], name
        for f in frames:
            assert f["fcs"] in (None, len(g[name][0])) or len(frames) > 1, name
            for b in f["blocks"]:
                seen["types"].add(b["type"])
                if b["type"] == "compressed":
                    seen["lit"].add(b["literals"]["mode"])
                    seen["trees"].add(b["literals"]["tree"])
                    if b["nseq"]:
                        seen["modes"].update(b["modes"])
                        assert len(b["sequences"]) == b["nseq"], name
                        assert b["count_form"] == (1 if b["nseq"] < 128 else 2 if b["nseq"] < 0x7F00 else 3), name
                    if b["literals"]["mode"] in ("huf", "treeless"):
                        assert 1 <= b["literals"]["max_code_len"] <= 11 and b["literals"]["streams"] in (1, 4), name
    # libzstd's streams use what this project's encoder never writes, and the reader follows
    assert {"predefined", "fse", "rle"} <= seen["modes"] and {"raw", "huf", "treeless"} <= seen["lit"]
    assert "compressed" in seen["types"] and seen["trees"] & {"direct", "fse"}


def test_valid_programs_replay_to_expand():
    n = 0
    for name, z, st, data, used in zf.verdicts():
        if st != 0:
            continue
        frames = zt.read(z)
        assert zt.replay(frames) == data, name
        n += 1
    assert n >= 300


def test_fields_of_written_programs():
    """frames written field by field come back field by field"""
    lits = zf.text(300, 5)
    fr = zf.Frame(window=0x68, fcs_bytes=4, checksum=True)
    body_seqs = [(10, 5, 10), (0, 4, 2), (3, 40, 1), (20, 300, 53)]
    fr.comp(lits, body_seqs, lit_mode="huf", lit_streams=4, lit_fse_weights=True, modes=("fse", "pre", "fse"))
    fr.rle(0x41, 1000)
    fr.raw(b"tail bytes", last=True)
    content = bytearray()
    lp = 0
    rep = [1, 4, 8]
    want = []
    for ll, ml, ofv in body_seqs:
        content += lits[lp:lp + ll]
        lp += ll
        before = tuple(rep)
        if ofv > 3:
            d = ofv - 3
            rep = [d, rep[0], rep[1]]
        else:
            idx = ofv - 1 + (ll == 0)
            d = rep[idx] if idx < 3 else rep[0] - 1
            if idx:
                rep = [d, rep[0], rep[2]] if idx == 1 else [d, rep[0], rep[1]]
        want.append((ll, ml, ofv, d, before))
        for _ in range(ml):
            content.append(content[-d])
    content += lits[lp:]
    content += b"\x41" * 1000 + b"tail bytes"
    fr.content = bytes(content)
    z = fr.bytes()
    assert zf.expand(z) == (0, bytes(content), len(z))
    f, = zt.read(z)
    assert (f["single"], f["window"], f["window_byte"], f["fcs"], f["fcs_bytes"], f["checksum"]) == (False, 8 << 20, 0x68, len(content), 4, True)
    assert f["checksum_value"] == zf.xxh64(bytes(content)) & 0xFFFFFFFF and f["header_bytes"] == 10 and f["size"] == len(z)
    b0, b1, b2 = f["blocks"]
    assert (b0["type"], b1["type"], b2["type"]) == ("compressed", "rle", "raw") and [b["last"] for b in f["blocks"]] == [False, False, True]
    assert (b1["size"], b1["content"], b2["content"]) == (1000, b"\x41" * 1000, b"tail bytes")
    li = b0["literals"]
    assert (li["mode"], li["streams"], li["tree"], li["regen"], li["size_format"]) == ("huf", 4, "fse", 300, 1) and li["max_code_len"] <= 11
    assert b0["lits"] == lits and b0["sequences"] == want
    assert (b0["nseq"], b0["count_form"], b0["modes"]) == (4, 1, ("fse", "predefined", "fse")) and b0["accuracy"][1] == 5
    assert zt.replay([f]) == bytes(content)
