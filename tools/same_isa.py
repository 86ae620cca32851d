#!/usr/bin/env python3
"""Is the device code of the working tree the same as that of a git revision?  Compiles each translation unit of the
working tree's build.py (its table of units) device-only to assembly (tools/kernel_resources.py: build.py's flags) for
both, drops the lines that carry the `__hip_cuid_<hash>` symbol (it hashes the input) and prints one verdict per file:
`identical`, or else the symbols whose text differs (exit status 1 if any file differs); a unit the revision does not
have is `new in the working tree` with its kernels listed, and no difference.  The check for a
change that is meant to move or rename code without touching what the compiler makes of it.
    python tools/same_isa.py [REVISION (default HEAD)] [-DSNK_PROFILE ...]"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

from kernel_resources import ROOT, SOURCES, device_asm


def sections(path):
    """{symbol: text} of an assembly file, cut at the labels in column 0 that are not local (.L...) ones"""
    out, name = {"": []}, ""
    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"([A-Za-z_$][\w$.]*):", line)
        if m:
            name = m.group(1)
            out.setdefault(name, [])
        out[name].append(line)
    return out


def main():
    rev = next((a for a in sys.argv[1:] if not a.startswith("-")), "HEAD")
    defines = [a for a in sys.argv[1:] if a.startswith("-")]
    status = 0
    with tempfile.TemporaryDirectory() as td:
        old = os.path.join(td, "old")
        os.mkdir(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "bullet-envs_amd", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        # (each tree is compiled with its own headers under its own names: a header renamed between the two is no difference)
        jobs = [(src, root, os.path.join(td, "%s_%d.s" % (tag, i))) for i, src in enumerate(SOURCES)
                for root, tag in ((old, "old"), (ROOT, "new"))]
        have = [os.path.exists(os.path.join(root, "bullet-envs_amd", src)) for src, root, out in jobs]
        with ThreadPoolExecutor(len(jobs)) as ex:
            [j.result() for j in [ex.submit(device_asm, root, defines, out, src) for (src, root, out), h in zip(jobs, have) if h]]
        for i, src in enumerate(SOURCES):
            if not have[2 * i] or not have[2 * i + 1]:
                side = 2 * i + 1 if have[2 * i + 1] else 2 * i
                kernels = sorted(k for k in sections(jobs[side][2]) if k.startswith("_Z") and "kernel" in k) if have[side] else []
                print("%s: %s (%d kernels: %s)" % (src, "new in the working tree" if have[2 * i + 1] else "only in " + rev,
                                                   len(kernels), " ".join(kernels)))
                continue
            a, b = sections(jobs[2 * i][2]), sections(jobs[2 * i + 1][2])
            differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
            if not differ and list(a) == list(b):
                print("%s: identical" % src)
                continue
            print("%s: %s" % (src, " ".join(differ) if differ else "same symbols, same text, another order"))
            status = 1
    return status


if __name__ == "__main__":
    sys.exit(main())
