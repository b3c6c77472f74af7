"""CPU tests of the refill of K1's two walks (minizip-ng_amd/csrc/inflate_walk.inc) in the 64-lane host emulation: a group
inside the input is one 16-byte load, the edge groups sit in a branch of their own, and one refill check per trip of four steps
may hand over both prefetched groups.  Once at the product's span limit and record caps, and once more with record caps and
spans so low that every window runs into them.  The cases are those of tests/walk_refill_cases.py; zlib is the judge of status,
bytes, consumed input and CRC, and tests/golden/k1_walk_refill_baseline.json holds what the refill of one group per check
behind selects, the code this one replaced, made of the cut streams.

The last test compiles tests/emul/k1_walk_main.cpp, a program of its own, with -fsanitize=address,undefined and runs it as
a child process: every case from a heap block that ends with the input's last aligned dword, at every misalignment.  (Not
with the input's last byte: a decoder may read the aligned dwords that hold a byte of the input whole, include/mzhip.h, and
mz_load_stream_dword does so for the last one.)"""
import hashlib
import json
import os
import time
import zlib

import pytest

from tests import k1_walk_emul
from tests import walk_refill_cases as W
from tests.k1_walk_emul import build_variant as _build_variant  # noqa: F401  (tests/test_gpu_walk_refill.py takes it from here)
from tests.test_kernel_emul import _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def builds():
    """{tag: library}: the product's span limit and record caps, and 512 bits / 16 / 8 steps"""
    return k1_walk_emul.builds()


def _check(tag, L, case, mis):
    name, z, data, want, used, cap = case
    st, iu, out, crc = _run(L.emul_inflate, z, cap, mis=mis, omis=(mis * 7 + 3) % 16)
    assert st == want, (tag, name, mis, st, want)
    if want == 0:
        assert iu == used and out == data and crc == zlib.crc32(data), (tag, name, mis, iu, used, len(out), len(data))


def test_every_misalignment(builds):
    """Every stream and both wide-step programs whole, the input at every misalignment 0 .. 15 inside patterned guard buffers
    (non-zero bytes behind the input): the last dword and the last group of four dwords take every phase."""
    t0 = time.time()
    cases = [c for c in W.everything() if c[3] == 0]
    assert len(cases) == 19
    assert {((mis & 3) + len(c[1])) % 16 for c in cases[:16] for mis in range(16)} == set(range(16))
    for tag, L in builds.items():
        for case in cases:
            for mis in range(16):
                _check(tag, L, case, mis)
    print("test_every_misalignment: %d builds x %d streams x 16, %.1f s" % (len(builds), len(cases), time.time() - t0))


def test_every_cut(builds):
    """Every stream cut at every byte of its last 48: status (and, should zlib still see an end, the consumed input) as zlib
    says.  The misalignment goes round with the cut, so that the cut end takes every phase of a group at every distance."""
    t0 = time.time()
    cases = [c for c in W.everything() if "/cut-" in c[0]]
    assert len(cases) == 17 * W.CUT_BYTES
    seen = set()
    for tag, L in builds.items():
        for k, case in enumerate(cases):
            mis = (k % W.CUT_BYTES) // 12 + 4 * (k % 4)          # (the low two bits stay for twelve cuts in a row: twelve residues of the end)
            seen.add(((mis & 3) + len(case[1])) % 16)
            _check(tag, L, case, mis)
    assert seen == set(range(16))
    print("test_every_cut: %d builds x %d cuts, %.1f s" % (len(builds), len(cases), time.time() - t0))


def test_knobs_change_no_record(builds):
    """What the walks hand on is what the refill before this one handed on: status, consumed input, bytes and CRC of every
    case -- the cut streams included, where zlib pins the status alone -- are those recorded in
    tests/golden/k1_walk_refill_baseline.json from the build its provenance field names."""
    with open(os.path.join(ROOT, "tests", "golden", "k1_walk_refill_baseline.json")) as f:
        base = json.load(f)["cases"]
    cases = W.everything()[:19] + W.everything()[19::37]
    assert set(base) == {c[0] for c in cases} and len(base) == len(cases)
    for name, z, _, _, _, cap in cases:
        st, iu, out, crc = _run(builds["product"].emul_inflate, z, cap, mis=5)
        assert [st, iu, len(out), crc, hashlib.sha256(out).hexdigest()] == base[name], name


def test_sanitised_program(tmp_path):
    """tests/emul/k1_walk_main.cpp under AddressSanitizer and UBSan: every case at every misalignment of the input from a
    heap block that ends with the input's last aligned dword; any read behind it ends the child with an error report.  Its
    verdicts are zlib's."""
    t0 = time.time()
    cases = W.everything()
    for c, mis, st, ol, iu, crc in k1_walk_emul.run_sanitised(tmp_path, "in", [(c[1], c[5]) for c in cases]):
        name, z, data, want, used, _ = cases[c]
        assert st == want, (name, mis, st, want)
        if want == 0:
            assert (ol, iu, crc) == (len(data), used, zlib.crc32(data)), (name, mis)
    print("test_sanitised_program: %d cases x 16 misalignments, %.1f s" % (len(cases), time.time() - t0))
