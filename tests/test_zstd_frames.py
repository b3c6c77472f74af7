"""The Zstandard frame writer and the plain reader of tests/zstd_frames.py held against libzstd (ZSTD_decompress through
ctypes): every program and every payload by class -- valid with exact bytes, output too small (error 70 <-> -200), invalid --
and the committed streams of tests/golden/zstd_streams.json against regeneration.  The tests that need libzstd skip where it
does not load."""
import base64
import json

import pytest

from tests import zstd_frames as zf

needs_libzstd = pytest.mark.skipif(zf.LIBZSTD is None, reason="libzstd does not load on this machine")


def _class(st):
    return "valid" if st == 0 else "small" if st == zf.OUT_FULL else "invalid"


def test_program_names_are_unique_and_families_present():
    names = [v[0] for v in zf.verdicts()]
    assert len(names) == len(set(names)) and len(names) >= 550
    for prefix in ("hdr_", "fcs_", "skippable_", "block_", "lit_", "weights_", "treeless_", "huf_", "nseq_", "mode_", "al_",
                   "less_than_one_", "zero_repeat_chain_", "ll_code_", "ml_code_", "of_code_", "rep_", "copy_distance_", "copy_",
                   "checksum_"):
        members = [v for v in zf.verdicts() if v[0].startswith(prefix)]
        assert any(v[2] == 0 for v in members), prefix       # every family has a valid member
    for name in zf.LENIENT_JUDGE:
        assert any(v[0].startswith(name) and v[2] == zf.DATA_ERROR for v in zf.verdicts()), name


def test_status_split_of_the_invalid_programs():
    """which of -3 / -5 / -109 an invalid stream gets is this project's rule (include/mzhip.h), stated by expand()"""
    V = dict((v[0], v) for v in zf.verdicts())
    assert all(v[2] == zf.BUF_ERROR for n, v in V.items() if n.startswith("cut_") or n in ("trailing_1", "trailing_2", "trailing_3"))
    assert all(V[n][2] == zf.BUF_ERROR for n in ("block_raw_cut", "block_rle_cut", "block_compressed_cut", "skippable_cut_size",
                                                  "skippable_cut_body", "checksum_cut_0", "checksum_cut_3", "block_last_missing"))
    assert V["hdr_dictionary_7"][2] == V["hdr_dictionary_4_bytes"][2] == zf.UNSUPPORTED
    assert all(V[n][2] == zf.DATA_ERROR for n in ("bad_magic", "trailing_4", "hdr_reserved_bit", "block_reserved", "hdr_window_log_32",
                                                   "fcs_one_large", "fcs_one_small", "checksum_33_wrong", "copy_into_previous_frame",
                                                   "copy_before_frame_start", "copy_too_few_literals", "treeless_no_tree",
                                                   "treeless_across_frames", "mode_0_rep_nothing", "mode_1_rep_across_frames",
                                                   "al_0_10", "al_1_9", "al_2_10", "weights_incomplete", "huf_bits_left_over",
                                                   "huf_no_marker", "seq_no_marker", "nseq_0_with_tail", "lit_jump_lie_long"))
    assert zf.expand(b"") == (zf.BUF_ERROR, b"", 0)
    # what stands in front of the problem: the complete blocks
    assert V["frame_behind_failing_frame"][2:4] == (zf.DATA_ERROR, zf.text(900, 11)[:50])
    assert V["copy_into_previous_frame"][3] == zf.text(900, 11)[:120]


@needs_libzstd
def test_programs_against_libzstd():
    for name, z, st, data, used in zf.verdicts():
        cls, got = zf.judge(z, len(data) if st == 0 else 400000)
        if zf.lenient(name):
            assert (st, cls) == (zf.DATA_ERROR, "valid"), name        # the documented cases, and they stay what the list says
            continue
        assert cls == _class(st), (name, st, cls, got)
        if st == 0:
            assert got == data and used == len(z), name


@needs_libzstd
def test_out_cap_one_short_against_libzstd():
    for name, z, st, data, used in zf.verdicts():
        if st == 0 and 0 < len(data) <= 5000 and not zf.lenient(name):
            assert zf.judge(z, len(data) - 1)[0] == "small", name
            assert zf.expand(z, len(data) - 1)[0] == zf.OUT_FULL, name


@needs_libzstd
def test_payloads_against_libzstd_and_the_reader():
    assert len(zf.payloads()) >= 24
    for name, z, d in zf.payloads():
        assert zf.judge(z, len(d)) == ("valid", d), name
        assert zf.expand(z) == (0, d, len(z)), name
        assert zf.judge(z[:-1], len(d))[0] == "invalid" and zf.expand(z[:-1])[0] in (zf.BUF_ERROR, zf.DATA_ERROR), name
        assert zf.judge(z + b"tail", len(d))[0] == "invalid" and zf.expand(z + b"tail")[0] == zf.DATA_ERROR, name


def test_reader_on_the_committed_streams():
    g = zf.golden_inputs()
    with open(zf.GOLDEN) as f:
        streams = json.load(f)
    assert sorted(streams) == sorted(g) and sum(len(v) for v in streams.values()) < 256 * 1024
    for name, b64 in streams.items():
        z = base64.b64decode(b64)
        assert zf.expand(z) == (0, g[name][0], len(z)), name
    # the long text has several blocks and treeless literals
    assert len(g["text_300k_l1"][0]) > 2 * zf.BLOCK_MAX


@needs_libzstd
def test_golden_file_against_regeneration():
    with open(zf.GOLDEN) as f:
        assert json.load(f) == zf.make_golden()
