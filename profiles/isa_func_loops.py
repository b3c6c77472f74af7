#!/usr/bin/env python3
"""isa_loops.py for a device FUNCTION instead of a kernel (no GPU needed): the loops of a function that is not inlined --
mz_chase_walk, mz_chase_emit -- from the compiler's own assembly of the default `make` build, with the vector-ALU
instructions, selects, moves and vector-memory operations of each.  This is how the walk loops' refill is counted between GPU
runs (profiles/r9).  Extra -D flags may be appended.

    python profiles/isa_func_loops.py [function=mz_chase_walk] [min_instructions=100] [-DMZ_CRC_CHAINS=1 ...]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from resource_usage import make_flags, SRC  # noqa: E402


def function_body(text, func):
    """lines of the first function whose mangled name contains <length><func>, from its label to its .Lfunc_end"""
    pat = re.compile(r"^(_Z\w*?%d%s\w*):" % (len(func), re.escape(func)))
    start = next(i for i, l in enumerate(text) if pat.match(l))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    return pat.match(text[start]).group(1), text[start:end]


def is_op(t):
    t = t.strip()
    return bool(t) and not t.startswith(";") and not t.startswith(".") and not t.endswith(":")


def loops_of(body):
    """(label, depth, first line, last line) of every loop, found as isa_loops.py finds them"""
    label_at = [i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)]
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"Loop Header: Depth=(\d+)", l)
        if not m:
            continue
        lab_i = max(j for j in label_at if j <= i)
        lab = re.match(r"^\.(LBB\d+_\d+):", body[lab_i]).group(1)[1:]
        named = [j for j, t in enumerate(body) if j > lab_i and re.search(r"(Header=|Parent Loop )%s\b" % re.escape(lab), t)]
        if not named:
            continue
        last_block = max(j for j in label_at if j <= max(named))
        nxt = [j for j in label_at if j > last_block]
        loops.append((".L" + lab, int(m.group(1)), lab_i, (nxt[0] - 1) if nxt else len(body) - 1))
    return loops


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-D")]
    extra = [a for a in sys.argv[1:] if a.startswith("-D")]
    func = args[0] if args else "mz_chase_walk"
    floor = int(args[1]) if len(args) > 1 else 100
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = ["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, "-I" + os.path.join(ROOT, "include")] + make_flags() + extra + [SRC]
        subprocess.run(cmd, check=True, capture_output=True)
        text = open(out).read().splitlines()
    name, body = function_body(text, func)
    print("%s (%s): %d instructions" % (func, " ".join(extra) or "default build", sum(1 for t in body if is_op(t))))
    print("%-12s %5s %7s %6s %8s %6s %5s %8s %8s %7s %6s %7s" % ("loop", "depth", "instr", "valu", "branches", "waits", "lds", "vmem", "vmem_x4", "scratch", "moves", "selects"))
    for lab, depth, a, b in loops_of(body):
        ops = [t.split()[0] for t in body[a:b + 1] if is_op(t)]
        if len(ops) < floor:
            continue
        c = lambda p: sum(1 for o in ops if re.match(p, o))  # noqa: E731
        print("%-12s %5d %7d %6d %8d %6d %5d %8d %8d %7d %6d %7d" % (lab, depth, len(ops), c(r"v_"), c(r"s_cbranch"), c(r"s_waitcnt"), c(r"ds_"),
                                                                      c(r"global_|buffer_|flat_"), c(r"global_(load|store)_dwordx4"), c(r"scratch_"),
                                                                      c(r"v_mov"), c(r"v_cndmask")))


if __name__ == "__main__":
    main()
