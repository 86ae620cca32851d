#!/usr/bin/env python3
"""Is the device code of the working tree the same as that of a git revision?  Compiles csrc/snk_api.hip device-only to
assembly (tools/kernel_resources.py: build.py's flags) for both, drops the lines that carry the `__hip_cuid_<hash>` symbol
(it hashes the input) and prints `identical`, or else the symbols whose text differs (exit status 1).  The check for a
change that is meant to move or rename code without touching what the compiler makes of it.
    python tools/same_isa.py [REVISION (default HEAD)] [-DSNK_PROFILE ...]"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

from kernel_resources import ROOT, device_asm


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
    with tempfile.TemporaryDirectory() as td:
        old = os.path.join(td, "old")
        os.mkdir(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "bullet-envs_amd", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        with ThreadPoolExecutor(2) as ex:
            jobs = [ex.submit(device_asm, root, defines, os.path.join(td, tag + ".s")) for root, tag in ((old, "old"), (ROOT, "new"))]
            [j.result() for j in jobs]
        a, b = sections(os.path.join(td, "old.s")), sections(os.path.join(td, "new.s"))
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    if not differ and list(a) == list(b):
        print("identical")
        return 0
    print("\n".join(differ) if differ else "same symbols, same text, another order")
    return 1


if __name__ == "__main__":
    sys.exit(main())
