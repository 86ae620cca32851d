"""The bits the step kernels produce, pinned: sha256 over four gait env-steps of 2000 environments (outputs + final
states) for the three kernel families -- 16 links register-resident, 16 links on the streamed-row kernels, 32 links.
Arithmetic is deterministic here (no atomics in the data path, results independent of the schedule: the scheduler tests),
so an edit that is meant to leave the arithmetic alone (a re-layout, a register split, a fence, the stash experiment of
round 5) must leave these hashes alone, and an edit that is meant to change it changes them HERE, visibly, with the
reason in the commit.  `tools/bits_hash.py step` prints the same hashes for any library (SNK_LIB).

The pins (tests/golden/step_bits.json) are keyed by the toolchain and by libsnk.so.cmd, the step kernels' command line
alone (tests/bit_pins.py: the key, the skip under an unknown one, the comparison).  A mismatch names the parts that differ
(observations, rewards, done flags, substep counts, state, aux; "all": their concatenation).  The pinned key is round 6's
(hipcc of ROCm 7.2.0: HIP 7.2.26015, AMD clang 22.0.0git; build.py's flags); its "all" are round 5's pins (8e46618d...,
f48c5d83..., 25eb76a4...): the arithmetic of round 5's final build -- contact_order 0 takes the same path."""
import hashlib
import importlib
import os

import numpy as np
import pytest

import bit_pins

pytestmark = pytest.mark.gpu

PARTS = ("obs", "rew", "done", "substeps", "state", "aux")
# case -> (n_modules, SNK_FORCE_STREAMED)
CASES = {"16": (16, False), "16s": (16, True), "32": (32, False)}


def state_hashes(pkg, n, streamed):
    """{part: hash} + "all" for the pinned workload."""
    syn = importlib.import_module("bullet-envs_amd.synthetic")
    B = 2000
    st = pkg.Stepper(B, n_modules=n)
    st.reset()
    st.set_ground_friction((0.5 + np.arange(B) % 11 / 10.0).astype(np.float32))
    hs = {k: hashlib.sha256() for k in PARTS + ("all",)}
    for j in range(4):
        out = st.step(syn.gait_actions(np.arange(B), j, n // 2).astype(np.float32))
        for k, a in zip(PARTS[:4], out):
            raw = np.ascontiguousarray(a).tobytes()
            hs[k].update(raw)
            hs["all"].update(raw)
    S, X = st.get_state()
    for k, a in (("state", S), ("aux", X)):
        hs[k].update(a.tobytes())
        hs["all"].update(a.tobytes())
    st.close()
    return {k: h.hexdigest()[:16] for k, h in hs.items()}


def hashes(pkg, case):
    """state_hashes of a named case; the streamed-row one under SNK_FORCE_STREAMED=1, the caller's value put back after"""
    n, streamed = CASES[case]
    old = os.environ.get("SNK_FORCE_STREAMED")
    if streamed:
        os.environ["SNK_FORCE_STREAMED"] = "1"
    try:
        return state_hashes(pkg, n, streamed)
    finally:
        if streamed and old is None:
            del os.environ["SNK_FORCE_STREAMED"]
        elif streamed:
            os.environ["SNK_FORCE_STREAMED"] = old


@pytest.mark.parametrize("n,streamed", [(16, False), (16, True), (32, False)])
def test_state_hash_is_pinned(pkg, n, streamed):
    case = "%d%s" % (n, "s" if streamed else "")
    bit_pins.check("step", case, lambda: hashes(pkg, case))
