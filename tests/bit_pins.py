"""The pinned bits' common part: how a build is keyed, where each family's pins are stored, and the one comparison.

A pin belongs to ONE toolchain and flag set: another hipcc may contract FMAs or select instructions differently
without any arithmetic bug.  So the pins are keyed by what bullet-envs_amd/build.py left next to the library -- the stamp
files it exports as STAMPS: hipcc's version lines, then each translation unit's command line -- and a family's key covers
the toolchain and the units whose kernels it pins, a prefix of that list, no more: the step kernels' pins do not move
when a query unit's command does.  Under an unknown key a pin test SKIPS and says what to do instead of failing or
being re-pinned blindly; tests/test_bit_pin_keys.py (no GPU) fails when the default build's key is not in a store, so
that skip cannot come from an edit of build.py unnoticed.  tools/bits_hash.py prints the hashes and the stores' blocks.
"""
import collections
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKGDIR = os.path.join(os.path.dirname(HERE), "bullet-envs_amd")


# bullet-envs_amd/build.py as a module (the directory's name has a hyphen)
_spec = importlib.util.spec_from_file_location("snk_build", os.path.join(PKGDIR, "build.py"))
build_py = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build_py)

# family -> how many of build.py's STAMPS key it, its store under tests/golden/ ({key: {"built_by": the keyed text,
# "cases": {case: {part: hash}}}}), the test module with its workload (CASES and hashes(pkg, case)), and what to verify on
# a new toolchain before its bits are pinned
Family = collections.namedtuple("Family", "stamps store module verify")
FAMILIES = {
    "step": Family(2, "step_bits.json", "test_gpu_bits", "the parity tests"),
    "query": Family(4, "query_bits.json", "test_gpu_query_bits", "the query kernels' accuracy tests"),
    "dynamics": Family(5, "dynamics_bits.json", "test_gpu_dynamics_bits", "tests/test_gpu_dynamics.py"),
}


def key(stamps):
    """(key, the text it hashes) of the stamps' texts, in STAMPS' order"""
    txt = "\n".join(stamps)
    return hashlib.sha256(txt.encode()).hexdigest()[:12], txt


def built_key(family):
    """key() of the library that lies next to the package; (None, why) when a stamp is missing"""
    names = build_py.STAMPS[:FAMILIES[family].stamps]
    try:
        return key([open(os.path.join(PKGDIR, s)).read() for s in names])
    except OSError:
        return None, "%s are missing (a library not built by bullet-envs_amd/build.py)" % " / ".join(names)


def store(family):
    return os.path.join(HERE, "golden", FAMILIES[family].store)


def array_hashes(parts):
    """{part: sha256[:16]} of (part, array) pairs"""
    return {part: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16] for part, a in parts}


def check(family, case, got):
    """`got()`: {part: hash} of the case on this build, computed once its key is known to be pinned.  Every part of either
    side is compared, and a mismatch names those that differ."""
    k, txt = built_key(family)
    pinned = json.load(open(store(family)))
    if k not in pinned:
        pytest.skip("no pinned %s bits for this toolchain / flag set (key %s: %s).  Verify %s on it, then run `python "
                    "tools/bits_hash.py %s --pins` on the GPU box and add the block it prints to tests/golden/%s."
                    % (family, k, txt, FAMILIES[family].verify, family, FAMILIES[family].store))
    got, want = got(), pinned[k]["cases"][case]
    differ = sorted(p for p in set(got) | set(want) if got.get(p) != want.get(p))
    assert not differ, "%s %s: %s differ from the pinned bits (got %s)" % (family, case, ", ".join(differ), got)
