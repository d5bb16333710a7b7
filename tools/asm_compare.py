#!/usr/bin/env python3
"""Compare the gfx950 assembly of kernels_dec.hip and kernels_enc.hip between two source trees, kernel by
kernel and device function by device function (no GPU): `hipcc -S --offload-arch=gfx950` on both, the
instruction lines of every function compared after dropping comments, directives and the function
number in local labels.  Prints the functions that differ or are missing and the count of identical
ones; exit status 1 if a function of the first tree is not identical in the second.
usage: asm_compare.py PARENT_TREE [NEW_TREE]   (NEW_TREE defaults to this tree)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_s(tree, src, out):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(tree, "himg_amd", "csrc")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-Wno-unused-value",
                    "-I" + os.path.join(tree, "include"), "-I" + csrc, "-S", os.path.join(csrc, src), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return {n: b for n, b in out.items() if b and n.startswith("_Z")}


def main():
    parent = os.path.abspath(sys.argv[1])
    new = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT
    total = same = 0
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("kernels_dec.hip", "kernels_enc.hip"):
            a_s, b_s = os.path.join(tmp, "a.s"), os.path.join(tmp, "b.s")
            compile_s(parent, src, a_s)
            compile_s(new, src, b_s)
            a, b = functions(a_s), functions(b_s)
            for n, body in a.items():
                total += 1
                if b.get(n) == body:
                    same += 1
                else:
                    print("%s %s %s" % ("DIFFERS" if n in b else "MISSING", src, n))
            for n in b:
                if n not in a:
                    print("NEW %s %s (%d instructions)" % (src, n, len([t for t in b[n] if not t.endswith(":")])))
    print("identical: %d of %d functions of the parent" % (same, total))
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
