#!/usr/bin/env python3
"""Regenerates profiles/r15_rows_stages.txt on a machine with an MI355X: runs tests/test_gpu_rows.py with SNK_GATE_SOFT=1 (every
gate printed, none asserted) and keeps its GATE and DIAG lines.
    python tools/rows_stages.py"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    env = dict(os.environ, SNK_GATE_SOFT="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_rows.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"],
                         cwd=ROOT, env=env, capture_output=True, text=True).stdout
    lines = [m.group(0).rstrip() for m in re.finditer(r"(GATE [A-E] |DIAG ).*", out)]
    head = ["tests/test_gpu_rows.py on one MI355X (tools/rows_stages.py: SNK_GATE_SOFT=1, every gate printed, none asserted):",
            "|gpu - ref|_inf / |ref|_inf per row or vector over a set; GPU | the float32 yardstick | ratio | limit", ""]
    with open(os.path.join(ROOT, "profiles", "r15_rows_stages.txt"), "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("%d lines, %d beyond a gate" % (len(lines), sum("OVER" in x for x in lines)))


if __name__ == "__main__":
    main()
