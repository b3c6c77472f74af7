"""CPU tests of two parts of K1 in the 64-lane host emulation of the shipped sources: the chase of pass 2 (inflate_walk.inc: a chase
takes its next target in front of a trip, a step only ever stops a chase) and the set-up of the near batches (inflate_commit.inc:
the rank searches on byte offsets with a scalar first step, the short-period prologue from a packed constant).  At the product's
span limit and record caps and once more with caps and spans so low that every window runs into them.  The cases are those of
tests/chase_lean_cases.py; zlib is the judge of status, bytes, consumed input and CRC.

The last test compiles tests/emul/k1_walk_main.cpp, a program of its own, with -fsanitize=address,undefined and runs it as
a child process over the same cases."""
import time
import zlib

import pytest

from tests import chase_lean_cases as CL
from tests import k1_walk_emul
from tests.test_kernel_emul import _run


@pytest.fixture(scope="module")
def builds():
    """{tag: library}: the product's span limit and record caps, and 512 bits / 16 / 8 steps"""
    return k1_walk_emul.builds()


def test_cases_are_zlibs():
    """the expected bytes of every case are what zlib makes of its stream, and zlib sees its end at the stream's last byte"""
    names = set()
    for name, z, data, cap in CL.everything():
        d = zlib.decompressobj(-15)
        assert d.decompress(z) == data and d.eof and d.unused_data == b"", name
        assert cap >= len(data)
        names.add(name)
    assert len(names) == len(CL.everything())
    assert {"retarget/flat8-cap2", "retarget/short-codes-cap1", "near/D3/lits0", "near/D7/run"} <= names


def _check(tag, L, case, mis, omis):
    name, z, data, cap = case
    st, iu, out, crc = _run(L.emul_inflate, z, cap, mis=mis, omis=omis)
    assert st == 0, (tag, name, mis, omis, st)
    if out != data:
        bad = next((k for k in range(min(len(out), len(data))) if out[k] != data[k]), min(len(out), len(data)))
        raise AssertionError("%s: %s (mis %d, omis %d): byte %d of %d differs (got %d bytes)" % (tag, name, mis, omis, bad, len(data), len(out)))
    assert iu == len(z) and crc == zlib.crc32(data), (tag, name, mis, omis, iu, len(z))


def test_retarget_cases(builds):
    """every retarget case through every build: small spans, long steps, block ends and both record caps"""
    t0 = time.time()
    cases = [c for c in CL.everything() if c[0].startswith("retarget/")]
    assert len(cases) == 57
    for tag, L in builds.items():
        for k, case in enumerate(cases):
            _check(tag, L, case, (k * 5) % 16, (k * 3 + 1) % 16)
    print("test_retarget_cases: %d builds x %d cases, %.1f s" % (len(builds), len(cases), time.time() - t0))


def test_near_cases_every_staging_phase(builds):
    """every near case with the output pointer at the misalignments that put the chunk's first byte at staging index 0, 1, 15
    (and the piece behind 0 / 1 / 15 / 16 fresh literals at 0 .. 31) -- the staging index of a byte is its offset in the chunk
    plus the 16-byte misalignment of where the chunk lands"""
    t0 = time.time()
    cases = [c for c in CL.everything() if c[0].startswith(("near/", "tails/"))]
    assert len(cases) == 77
    for tag, L in builds.items():
        for k, case in enumerate(cases):
            for omis in ((0, 1, 15) if not tag.endswith("_caps") else ((k * 7) % 16,)):
                _check(tag, L, case, (k * 3) % 16, omis)
    print("test_near_cases_every_staging_phase: %d builds x %d cases, %.1f s" % (len(builds), len(cases), time.time() - t0))


def test_knobs_change_no_result(builds):
    """status, bytes, consumed input and CRC of every case at one more pair of pointers are zlib's"""
    for k, case in enumerate(CL.everything()):
        _check("product", builds["product"], case, 5, (k * 11) % 16)


def test_sanitised_program(tmp_path):
    """tests/emul/k1_walk_main.cpp under AddressSanitizer and UBSan: every case at sixteen output misalignments from heap
    blocks that end with the input's last aligned dword and the output's capacity.  Its verdicts are zlib's."""
    t0 = time.time()
    cases = [c for c in CL.everything() if len(c[2]) <= 40000]        # (the sanitised emulation is slow: the long runs once, below)
    cases += [c for c in CL.everything() if len(c[2]) > 40000][:2]
    for c, omis, st, ol, iu, crc in k1_walk_emul.run_sanitised(tmp_path, "out", [(c[1], c[3]) for c in cases]):
        name, z, data, _ = cases[c]
        assert (st, ol, iu, crc) == (0, len(data), len(z), zlib.crc32(data)), (name, omis, st, ol, iu)
    print("test_sanitised_program: %d cases x 16 misalignments, %.1f s" % (len(cases), time.time() - t0))
