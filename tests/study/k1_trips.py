"""Design study next to k1_steps.py: how often one span window of K1 runs the loops whose cost is counted per trip or per batch --
trips of four steps of pass 1 and pass 2, targets a chase takes behind its first, far and near batches of the commit -- counted
by the host emulation of the shipped kernel source built with -DMZ_STATS (counters 5, 7, 25, 26, 27), on 200 x 64 KiB of the
bench corpus at level 6.  With profiles/isa_func_loops.py this recomputes a window's instruction budget without a GPU.  Not
part of the product or the test suite.

    python tests/study/k1_trips.py [extra -D flags, e.g. -DMZ_CHASE_SMAX=512u]
"""
import ctypes as C
import os
import random
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import synth  # noqa: E402


def main():
    flags = sys.argv[1:]
    so = "/tmp/libemul_trips_%s.so" % (abs(hash(tuple(flags))) % 10 ** 8)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-DMZHIP_HOST_EMUL", "-DMZ_STATS",
                           "-I" + os.path.join(ROOT, "minizip-ng_amd", "csrc"), "-I" + os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "emul", "emul.cpp"), "-o", so])
    L = C.CDLL(so)
    L.emul_stats.restype = C.POINTER(C.c_ulonglong)
    text, desc = synth.bench_corpus()
    rnd = random.Random(5)
    for _ in range(200):
        o = rnd.randrange(0, len(text) - 65536)
        d = text[o:o + 65536]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        z = co.compress(d) + co.flush()
        out = C.create_string_buffer(len(d) + 64)
        ol, iu, crc = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = L.emul_inflate(z, len(z), out, len(d), C.byref(ol), C.byref(iu), C.byref(crc))
        assert st == 0 and out.raw[:ol.value] == d
    s = L.emul_stats()
    win = s[8]
    print("%s, 200 x 64 KiB at level 6; flags %s" % (desc, " ".join(flags) or "(default)"))
    print("windows %d; trips of four steps per window: pass 1 %.1f, pass 2 %.1f (targets a chase took behind its first: %.1f per window); "
          "far batches %.1f, near batches %.1f per window" % (win, s[5] / 4.0 / win, s[7] / 4.0 / win, s[27] / win, s[26] / win, s[25] / win))


if __name__ == "__main__":
    main()
