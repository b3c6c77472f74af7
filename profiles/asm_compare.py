#!/usr/bin/env python3
"""Compare the device assembly of two trees function by function (no GPU needed): which kernels and device functions a
change left instruction for instruction alone, and by how much the others moved.  Both trees are compiled with the flags of
their own default `make` (hipcc --cuda-device-only -S); a file that ends in .s is taken as that assembly instead.

    python profiles/asm_compare.py PARENT_TREE_OR_S [HEAD_TREE_OR_S = this tree] > profiles/r11/asm_compare.txt

Of every function the text between its label and its end is kept, without comment lines, trailing comments, directives and
label definitions, and with the numbers of local labels (.LBB3_17) blanked.  Register names are NOT normalised: once the
allocator shifts one register, most lines of a function differ, and the count of differing lines says nothing about the
cause.  Functions are paired by name and template arguments, not by parameter types (a kernel whose argument struct was
renamed is still the same kernel).  For a function that differs in few lines the mnemonics of those lines are listed.  The
resource figures the compiler prints behind every function are compared as well.  The script compares text; it knows no
instruction.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEW = 40  # list the mnemonics of the differing lines up to this many
RES = (("sgpr", r"^; TotalNumSgprs: (\d+)"), ("vgpr", r"^; NumVgprs: (\d+)"), ("agpr", r"^; NumAgprs: (\d+)"),
       ("scratch", r"^; ScratchSize: (\d+)"), ("lds", r"^; LDSByteSize: (\d+)"), ("occ", r"^; Occupancy: (\d+)"))


def assembly(arg, tmp, tag):
    if arg.endswith(".s"):
        return open(arg).read().splitlines()
    csrc = os.path.join(arg, "minizip-ng_amd", "csrc")
    make = subprocess.run(["make", "-C", csrc, "-n", "-B"], capture_output=True, text=True).stdout
    line = next(l for l in make.splitlines() if "hipcc" in l and "mzhip_kernels.hip" in l)
    flags = [t for t in line.split() if t.startswith(("-D", "-O", "-std", "--offload-arch", "-f"))]
    out = os.path.join(tmp, tag + ".s")
    subprocess.run(["hipcc", "--cuda-device-only", "-S", "-o", out] + flags + [os.path.join(csrc, "mzhip_kernels.hip")],
                   check=True, capture_output=True)
    return open(out).read().splitlines()


def key_of(mangled):
    """k_inflate_batch<ILb0E> from _Z15k_inflate_batchILb0EEv11InflateArgs: the name and its template arguments"""
    m = re.match(r"_ZL?(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    base, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    t = re.match(r"I(.*?E)E", rest)
    return base + ("<%s>" % t.group(1) if t else "")


def normal(line):
    t = line.split(";", 1)[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return None
    return re.sub(r"\.L([A-Za-z_]+)\d+(_\d+)?", r".L\1", t)


def functions(text):
    """{key: (instructions, resources)} in file order"""
    out, i = {}, 0
    while i < len(text):
        m = re.match(r"^(_Z\w+):", text[i])
        if not m or i == 0 or "@function" not in "".join(text[max(0, i - 4):i]):
            i += 1
            continue
        end = next(j for j in range(i, len(text)) if text[j].startswith(".Lfunc_end"))
        body = [t for t in (normal(l) for l in text[i + 1:end]) if t]
        res = {}
        for l in text[end:end + 60]:
            for k, pat in RES:
                g = re.match(pat, l)
                if g and k not in res:
                    res[k] = int(g.group(1))
        key = key_of(m.group(1))
        out[key if key not in out else m.group(1)] = (body, res)
        i = end + 1
    return out


def main():
    args = sys.argv[1:]
    if not args:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        parent = functions(assembly(args[0], tmp, "parent"))
        head = functions(assembly(args[1] if len(args) > 1 else ROOT, tmp, "head"))
    same = [k for k in parent if k in head and parent[k][0] == head[k][0]]
    print("%d functions in the parent, %d in the head, %d instruction for instruction the same:" % (len(parent), len(head), len(same)))
    for k in same:
        print("  = %-34s %6d" % (k, len(parent[k][0])))
    print("\ndiffering (instructions parent -> head, lines of the parent replaced or dropped / lines of the head new):")
    for k in parent:
        if k not in head or k in same:
            continue
        a, b = parent[k][0], head[k][0]
        minus, plus = [], []
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
            if tag != "equal":
                minus += a[i1:i2]
                plus += b[j1:j2]
        print("  ~ %-34s %6d -> %6d   -%d / +%d" % (k, len(a), len(b), len(minus), len(plus)))
        if len(minus) + len(plus) <= FEW:
            print("      mnemonics of those lines: %s" % " ".join(sorted({t.split()[0] for t in minus + plus})))
    for k in parent:
        if k not in head:
            print("  - %s (only in the parent)" % k)
    for k in head:
        if k not in parent:
            print("  + %s (only in the head)" % k)
    print("\nresources (SGPRs, VGPRs, AGPRs, scratch bytes per lane, static LDS bytes, occupancy) that moved:")
    moved = 0
    for k in parent:
        if k in head and parent[k][1] != head[k][1]:
            moved += 1
            print("  %-34s %s" % (k, "  ".join("%s %s -> %s" % (n, parent[k][1].get(n), head[k][1].get(n)) for n, _ in RES
                                                  if parent[k][1].get(n) != head[k][1].get(n))))
    if not moved:
        print("  none")
    return 0


if __name__ == "__main__":
    sys.exit(main())
