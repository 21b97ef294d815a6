#!/usr/bin/env python
"""One line per kernel of libcoot_hip.so: file, name, instruction lines and a hash of the normalised assembly (no GPU needed).
    python tools/kernel_isa.py [--f16] > A.txt     build.sh's flags plus --cuda-device-only -S, for every csrc/*.hip
    python tools/kernel_isa.py A.txt B.txt         the kernels that differ, by name, and the ones only one table has
A body runs from the kernel's label to its .Lfunc_end, without comments and blank lines, and with .LBB<n>_<m> written as .LBB_<m>
(n is the function's index in its file).  The lines are hashed as text: a refactor that moves kernels shows its code did not change."""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from kernel_resources import CSRC, demangle

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -munsafe-fp-atomics -Wno-unused-result --cuda-device-only -S -o -".split()


def kernels(f, extra):
    asm = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + [f], cwd=CSRC, capture_output=True, text=True, check=True).stdout.split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel (\S+)", line) for line in asm) if m}
    rows, cur, body = [], None, []
    for line in asm:
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur, body = line[:-1], []
        elif line.startswith(".Lfunc_end"):
            text = "\n".join(body)
            rows.append((f, cur, sum(1 for b in body if not b.startswith(".") and not b.endswith(":")), hashlib.sha256(text.encode()).hexdigest()[:16]))
            cur = None
        elif line:
            body.append(line)
    return rows


def table(extra):
    files = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    with ThreadPoolExecutor(8) as pool:
        rows = [r for part in pool.map(lambda f: kernels(f, extra), files) for r in part]
    for (f, _, n, h), name in zip(rows, demangle([r[1] for r in rows])):
        print(f"{f:22s} {n:7d} {h}  {name}")
    print(f"# {len(rows)} kernels")


def load(path):  # name -> (instruction lines, hash): the file may change, the name may not
    with open(path) as fh:
        return {p[3]: (p[1], p[2]) for p in (line.rstrip("\n").split(None, 3) for line in fh if not line.startswith("#")) if len(p) == 4}


def compare(a, b):
    A, B = load(a), load(b)
    for k in sorted(A.keys() & B.keys()):
        if A[k] != B[k]:
            print(f"differs  {k}: {A[k][0]} lines {A[k][1]} -> {B[k][0]} lines {B[k][1]}")
    for k in sorted(A.keys() - B.keys()):
        print(f"only in {a}: {k}")
    for k in sorted(B.keys() - A.keys()):
        print(f"only in {b}: {k}")
    print(f"{len(A)} kernels in {a}, {len(B)} in {b}, {sum(A[k] == B[k] for k in A.keys() & B.keys())} identical")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--f16"]
    sys.exit(compare(*args) if len(args) == 2 else table(["-DCOOT_OPERAND_F16"] if "--f16" in sys.argv else []))
