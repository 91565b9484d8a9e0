#!/usr/bin/env python3
"""Per-kernel digest of a .hip file's gfx950 instruction stream, to compare two revisions of a kernel file:
`python tools/isa_digest.py ader_amd/csrc/FILE.hip [-DADER_XCHECK ...]` compiles FILE with ader_amd/build.py's flags for it and prints
one line per kernel: demangled name, lines of its instruction stream with its descriptor (comments and blank lines stripped), sha256
of those lines (without the kernel's own name and the per-function number in local labels, which shifts when a neighbour comes or goes)."""
import hashlib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ader_amd.build import COMMON, EXTRA, HIPCC  # noqa: E402


def digest(src, defines=()):
    cmd = [HIPCC] + COMMON + EXTRA.get(os.path.basename(src), []) + list(defines) + ["--offload-device-only", "-S", src, "-o", "-"]
    asm = subprocess.run(cmd, stdout=subprocess.PIPE, check=True).stdout.decode()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur, body = [], None, []
    for line in asm.splitlines():
        line = re.sub(r"^\.section\s+\.text\..*", ".text", line.split(";")[0].strip())       # (a template's own section)
        m = re.match(r"(\S+):$", line)
        if m and m.group(1) in kernels:
            cur, body = m.group(1), []
        elif cur and line.startswith(".Lfunc_end"):
            out.append((cur, len(body), hashlib.sha256("\n".join(body).encode()).hexdigest()))
            cur = None
        elif cur and line:
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line).replace(cur, "@"))     # (its own name: in the kernel descriptor's head)
    names = subprocess.run(["c++filt"] + [k for k, _, _ in out], stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    plain = lambda m: m.group(2)[:int(m.group(1))]              # a name c++filt does not know (bf16 arguments): its first component
    return [(re.sub(r"^_Z(\d+)(\w+)$", plain, re.sub(r"^void |\(.*$", "", nm)), n, h) for nm, (_, n, h) in zip(names, out)]


if __name__ == "__main__":
    for name, n, h in sorted(digest(sys.argv[1], sys.argv[2:])):
        print("%-40s %7d  %s" % (name, n, h))
