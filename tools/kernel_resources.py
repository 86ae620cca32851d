#!/usr/bin/env python3
"""Registers, scratch bytes per lane and occupancy of every kernel of libsnk.so, as the compiler reports them: a device-only
compile of csrc/snk_api.hip to assembly with build.py's flags (35 s), the `; NumVgprs / ScratchSize / Occupancy` comments
of each kernel.  The numbers DESIGN.md 5 / 8 quote come from here (profiles/r05_kernel_resources.txt).
    python tools/kernel_resources.py [-DSNK_V1_RESN=48 ...]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bullet-envs_amd"))
from build import SOURCES      # noqa: E402  (the library's translation units, the working tree's: build.py's table)


def device_asm(root, args, out, src=SOURCES[0]):
    """Compiles <root>/bullet-envs_amd/<src> (the step kernels' translation unit; main() lists every unit of
    build.py's table) device-only to assembly with the product's own flags (that tree's
    `build.py --print-flags`) plus `args`; returns the command.  (tools/same_isa.py compares two trees with it.)"""
    pkg = os.path.join(root, "bullet-envs_amd")
    flags = subprocess.check_output([sys.executable, os.path.join(pkg, "build.py"), "--print-flags"], text=True).split()
    cmd = ["/opt/rocm/bin/hipcc"] + flags + list(args) + ["--offload-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, cwd=pkg, check=True, stderr=subprocess.DEVNULL)
    return cmd


def main():
    print("%-46s %6s %6s %9s %5s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "occ"))
    for src in SOURCES:
        one(src)


def one(src):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "snk.s")
        cmd = device_asm(ROOT, sys.argv[1:], out, src)
        lines = open(out).read().split("\n")
    print("# " + " ".join(cmd[:-2]))
    name = None
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN3snk\w+):\s*; @", l)
        if m:
            name = m.group(1)
        m = re.match(r"; ScratchSize: (\d+)", l)
        if m and name and "kernel" in name:
            blk = "\n".join(lines[i - 14:i + 14])
            g = lambda k: (re.search(r"; %s: (\d+)" % k, blk) or [None, "?"])[1]      # noqa: E731
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            short = re.sub(r"\(.*", "", dem).replace("void snk::", "")
            print("%-46s %6s %6s %9s %5s" % (short, g("NumVgprs"), g("NumSGPRsForWavesPerEU"), m.group(1), g("Occupancy")))
            name = None


if __name__ == "__main__":
    main()
